// device_api.hip -- the device half of the C ABI (include/dsrt.h): context, scene upload + re-layout,
// render launch, tile de-interleave, and the reference's own entry points on top of them.
//
// Replaces: the cudaMalloc/cudaMemcpy half of build_gpu_scene (src/gpu_scene_builder.cpp:322-331, 475-546),
// free_gpu_scene (:603-626) and the host launcher gpu_render_scene (src/gpu_render.cu:1037-1108).
// Differences by design: the scene is converted once into the traversal layout of device_layout.h and stays
// resident across frames (the reference re-uploads everything per frame, src/main.cpp:405); errors are returned,
// not only printed; the launch is asynchronous on a caller-supplied stream; output goes to caller-owned buffers.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cassert>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/dsrt.h"
#include "../host/host_internal.hpp"
#include "device_layout.h"
#include "hip_check.h"
#include "launchers.h"

namespace dsrt {
const RenderLaunchers& render_launchers(bool device_libm) { return device_libm ? devlibm::compiled_render_launchers() : compiled_render_launchers(); }
}  // namespace dsrt

using namespace dsrt;

namespace {

// Frames in flight on separate streams (dsrt_ctx_clone, dsrt_multi_render_sequence) only overlap on the device if each stream
// gets a hardware queue of its own; the HIP runtime maps streams onto 4 unless told otherwise BEFORE it initialises.  The
// library asks for 16 in its first dsrt_device_count / dsrt_ctx_create call -- documented there in include/dsrt.h; not at load time, so
// that loading the library changes nothing in the host process -- unless the host has set the variable itself.  (No effect if HIP is
// already up.)
void hw_queues_default() {
    static std::once_flag once;
    std::call_once(once, [] { (void)setenv("GPU_MAX_HW_QUEUES", "16", 0); });
}

template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    ~DevBuf() { reset(); }
    void reset() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
    int upload(const std::vector<T>& v) {
        reset();
        if (v.empty()) return DSRT_OK;
        HIP_TRY(hipMalloc((void**)&p, v.size() * sizeof(T)));
        n = v.size();
        HIP_TRY(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
        return DSRT_OK;
    }
    int alloc(size_t count) {
        reset();
        if (!count) return DSRT_OK;
        HIP_TRY(hipMalloc((void**)&p, count * sizeof(T)));
        n = count;
        return DSRT_OK;
    }
    int grow(size_t count) { return n < count ? alloc(count) : DSRT_OK; }      // contents are not kept
};

// What changes from frame to frame: set by an upload, replaced per context by dsrt_scene_set_camera_sun and the drop-in.
struct FrameState {
    GPUCamera camera{};
    DsrtF3 sun_dir{}, sun_radiance{};
    int sun_enabled = 0;
};
FrameState frame_of(const GPUScene& s) { return FrameState{s.camera, s.sun_dir, s.sun_radiance, s.sun_enabled ? 1 : 0}; }

// What dsrt_scene_upload_bodies keeps resident beside the scene for dsrt_scene_set_body_poses (launchers.h, BodiesView; layout: DESIGN.md).
struct BodiesResident {
    int n_bodies = 0;
    DevBuf<float4> rest_v, rest_n, pair_box;
    DevBuf<float> poses, pads, root_box;
    DevBuf<int2> refit;
    DevBuf<int4> chain;
    std::vector<int> entry_start;                  // n_bodies + 1: body b's movable entries are [entry_start[b], entry_start[b + 1])
    std::vector<int2> depth_range;                 // {first, count} into `refit`, one per depth that has movable records, deepest first
    BodiesView view{};
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    float last_ms[3] = {0, 0, 0};
    ~BodiesResident() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
};

// The scene in traversal layout, owning its device memory.
struct PackedScene {
    DevBuf<float4> pairs, tri_pairs, tri_shade, tri_uv, tri_cert, materials;
    DevBuf<uint8_t> pair_depth;
    DevBuf<int2> big_leaves;
    DevBuf<GPUSphere> spheres;
    DevBuf<GPUTextureHeader> tex_headers;
    DevBuf<float> tex_pool;
    DeviceScene view{};
    FrameState frame;
    bool has_second_tree = false;   // the certified second tree is resident (pack_scene)
    float scene_extent = 0.0f, scene_centre[3] = {0, 0, 0};
    bool lean = false;              // no spheres, no textures, Lambertian materials only: the production launches use the kernels' LEAN instantiation (path_machine.h)
    bool valid = false;
    std::unique_ptr<BodiesResident> bodies;   // uploaded with dsrt_scene_upload_bodies
};

float4 as_f4(float a, float b, float c, float d) { return make_float4(a, b, c, d); }

// The 12-float camera block of FrameParams / BatchFrame / GBufferArgs (device_layout.h, kCamOrigin ...).
void pack_camera(const GPUCamera& c, float (&cam)[12]) {
    const float cam12[12] = {c.origin.x, c.origin.y, c.origin.z, c.lower_left_corner.x, c.lower_left_corner.y, c.lower_left_corner.z,
                             c.horizontal.x, c.horizontal.y, c.horizontal.z, c.vertical.x, c.vertical.y, c.vertical.z};
    std::memcpy(cam, cam12, sizeof cam12);
}

float bits(int i) { float f; std::memcpy(&f, &i, 4); return f; }

// Leaf size of the certified second tree (its structure is free: any tree over the reachable triangles will do).  Development override: DSRT_SECOND_TREE_LEAF=1..7.
int second_tree_leaf_max() {
    if (const char* e = std::getenv("DSRT_SECOND_TREE_LEAF")) { const long v = std::strtol(e, nullptr, 10); if (v >= 1 && v <= 7) return (int)v; }
    return 4;
}

// What packing one tree into the shared arrays yields.
struct PackedTree { int root_ref = kRefNone; int stack_need = 0; float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0}; };

// The arrays both trees are appended to (device_layout.h).  References are absolute: an internal reference is its record's index in `pairs` + kRefBias, a leaf
// reference carries the index of its first record in `isect`; `shade` / `uv` / `cert` grow in step with `isect` (two slots per pair record).
struct PackArrays {
    std::vector<float4> pairs, isect, shade, uv, cert;
    std::vector<int> depth_of_all;                                       // depth of every record of `pairs` (the counting build's histogram reads it)
    std::vector<int2> big;
};

// What pack_tree knows about where things went, for a caller that asks (dsrt_scene_upload_bodies): per node record its node and depth, per pair record its one or
// two source triangles (-1 = none).  A leaf's first pair record is in its reference.
struct PackReport { std::vector<int> record_node, record_depth; std::vector<int2> pair_src; };

// Appends the tree (nodes, tri_indices) over the scene's triangles.  Validates every index the kernel will follow, so the fast (unchecked) kernel build never sees
// an out-of-range reference.  `cert_boxes` (null, or 6 floats per TRIANGLE): appended per slot to arr.cert -- the certified second tree's records.
int pack_tree(const GPUScene& h, const GPUBVHNode* nodes, int M, const int* tri_indices, int n_indexed, bool textured, const float* cert_boxes, PackArrays& arr, PackedTree& out,
              PackReport* report = nullptr) {
    const int N = h.num_triangles;
    for (int i = 0; i < n_indexed; ++i) if (tri_indices[i] < 0 || tri_indices[i] >= N) { set_error("tri_indices entry out of range"); return DSRT_ERR_INVALID; }
    // internal node -> slot in `pairs`, assigned in a depth-first walk from the root (also detects cycles / sharing)
    const int base = (int)(arr.pairs.size() / 4);
    std::vector<int> slot_of(M, -1);
    std::vector<char> seen(M, 0);
    struct Item { int node; int internal_above; };
    std::vector<Item> todo{{0, 0}};
    int stack_need = 0;
    std::vector<int> order;                                          // internal nodes in visiting order
    std::vector<int> depth_of;                                       // ... and their depth (root = 0)
    while (!todo.empty()) {
        Item it = todo.back(); todo.pop_back();
        if (it.node < 0 || it.node >= M) { set_error("BVH child index out of range"); return DSRT_ERR_INVALID; }
        if (seen[it.node]) { set_error("BVH is not a tree (node reached twice)"); return DSRT_ERR_INVALID; }
        seen[it.node] = 1;
        const GPUBVHNode& n = nodes[it.node];
        if (n.tri_count > 0) {
            if (n.tri_offset < 0 || (long long)n.tri_offset + n.tri_count > n_indexed) { set_error("BVH leaf range out of bounds"); return DSRT_ERR_INVALID; }
            if (it.internal_above > stack_need) stack_need = it.internal_above;
        } else {
            slot_of[it.node] = (int)order.size();
            order.push_back(it.node);
            depth_of.push_back(it.internal_above);
            todo.push_back({n.right, it.internal_above + 1});
            todo.push_back({n.left, it.internal_above + 1});
        }
    }
    if (stack_need > 64) { set_error("BVH needs a traversal stack deeper than the reference's 64 entries"); return DSRT_ERR_BVH_DEPTH; }
    // Triangle storage: every leaf gets ceil(count / 2) pair records of its own, filled in tri_indices order.
    auto emit_leaf = [&](const GPUBVHNode& n) -> int {
        const int first_pair = (int)(arr.isect.size() / 5);
        for (int i = 0; i < n.tri_count; i += 2) {
            float q[2][9] = {{0}};
            for (int w = 0; w < 2; ++w) {
                const bool real = i + w < n.tri_count;
                const int src = real ? tri_indices[n.tri_offset + i + w] : -1;
                float4 s0 = as_f4(0, 0, 0, 0), s1 = s0, s2 = as_f4(0, bits(0), bits(-1), bits(-1)), u0 = s0, u1 = s0, c0 = s0, c1 = s0;
                if (real) {
                    const GPUTriangle& t = h.triangles[src];
                    const float v[9] = {t.v0.x, t.v0.y, t.v0.z, t.v1.x - t.v0.x, t.v1.y - t.v0.y, t.v1.z - t.v0.z, t.v2.x - t.v0.x, t.v2.y - t.v0.y, t.v2.z - t.v0.z};
                    std::memcpy(q[w], v, sizeof v);
                    s0 = as_f4(t.n0.x, t.n0.y, t.n0.z, t.n1.x);
                    s1 = as_f4(t.n1.y, t.n1.z, t.n2.x, t.n2.y);
                    s2 = as_f4(t.n2.z, bits(t.material_id), bits(t.albedo_tex), bits(src));
                    u0 = as_f4(t.uv0.x, t.uv0.y, t.uv1.x, t.uv1.y);
                    u1 = as_f4(t.uv2.x, t.uv2.y, 0.0f, 0.0f);
                    if (cert_boxes) { const float* cb = cert_boxes + 6 * (size_t)src; c0 = as_f4(cb[0], cb[1], cb[2], cb[3]); c1 = as_f4(cb[4], cb[5], 0.0f, 0.0f); }
                }
                arr.shade.push_back(s0); arr.shade.push_back(s1); arr.shade.push_back(s2);
                if (textured) { arr.uv.push_back(u0); arr.uv.push_back(u1); }
                if (cert_boxes) { arr.cert.push_back(c0); arr.cert.push_back(c1); }
            }
            arr.isect.push_back(as_f4(q[0][0], q[1][0], q[0][1], q[1][1]));
            arr.isect.push_back(as_f4(q[0][2], q[1][2], q[0][3], q[1][3]));
            arr.isect.push_back(as_f4(q[0][4], q[1][4], q[0][5], q[1][5]));
            arr.isect.push_back(as_f4(q[0][6], q[1][6], q[0][7], q[1][7]));
            arr.isect.push_back(as_f4(q[0][8], q[1][8], 0.0f, 0.0f));
            if (report) report->pair_src.push_back(make_int2(tri_indices[n.tri_offset + i], i + 1 < n.tri_count ? tri_indices[n.tri_offset + i + 1] : -1));
        }
        return first_pair;
    };
    auto ref_of = [&](int node) -> int {
        const GPUBVHNode& n = nodes[node];
        if (n.tri_count <= 0) return base + slot_of[node] + kRefBias;
        const int first_pair = emit_leaf(n);
        if (n.tri_count <= 7) return make_leaf_ref(n.tri_count - 1, first_pair);
        arr.big.push_back(make_int2(first_pair, n.tri_count));
        return make_leaf_ref(7, (int)arr.big.size() - 1);
    };
    arr.pairs.resize(((size_t)base + order.size()) * 4);
    for (size_t s = 0; s < order.size(); ++s) {
        const GPUBVHNode& n = nodes[order[s]];
        const GPUBVHNode& l = nodes[n.left];
        const GPUBVHNode& r = nodes[n.right];
        float4* rec = arr.pairs.data() + 4 * ((size_t)base + s);
        rec[0] = as_f4(l.bbox_min.x, r.bbox_min.x, l.bbox_max.x, r.bbox_max.x);
        rec[1] = as_f4(l.bbox_min.y, r.bbox_min.y, l.bbox_max.y, r.bbox_max.y);
        rec[2] = as_f4(l.bbox_min.z, r.bbox_min.z, l.bbox_max.z, r.bbox_max.z);
        const int ref_left = ref_of(n.left), ref_right = ref_of(n.right);          // in this order: leaf records follow the walk
        rec[3] = as_f4(bits(ref_left), bits(ref_right), l.bbox_min.x + l.bbox_max.x, r.bbox_min.x + r.bbox_max.x);   // the x sums of the ordering test, in float as the kernel would form them
    }
    arr.depth_of_all.insert(arr.depth_of_all.end(), depth_of.begin(), depth_of.end());
    if (report) { report->record_node = order; report->record_depth = depth_of; }
    const GPUBVHNode& root = nodes[0];
    out.lo[0] = root.bbox_min.x; out.lo[1] = root.bbox_min.y; out.lo[2] = root.bbox_min.z;
    out.hi[0] = root.bbox_max.x; out.hi[1] = root.bbox_max.y; out.hi[2] = root.bbox_max.z;
    out.root_ref = ref_of(0);
    out.stack_need = stack_need;
    return DSRT_OK;
}

// Host-side conversion of reference-layout arrays into the traversal layout.  `second_tree`: also build and pack the certified second tree (below).
int pack_scene(const GPUScene& h, PackedScene& out, bool second_tree, PackReport* report = nullptr) {
    const int N = h.num_triangles, M = h.num_bvh_nodes;
    if (N < 0 || M < 0 || h.num_spheres < 0 || h.num_materials < 0 || h.num_textures < 0 || h.texture_pool_floats < 0) {
        set_error("scene has a negative count"); return DSRT_ERR_INVALID;
    }
    if ((N && !h.triangles) || (h.num_spheres && !h.spheres) || (h.num_materials && !h.materials)) { set_error("scene array pointer is null"); return DSRT_ERR_INVALID; }
    if (N > (1 << 28)) { set_error("more than 2^28 triangles"); return DSRT_ERR_INVALID; }
    const bool has_bvh = h.bvh_nodes && M > 0 && h.tri_indices;        // bvh_hit_closest's own guard, src/gpu_render.cu:394-397
    for (int i = 0; i < N; ++i) if (h.triangles[i].material_id < 0 || h.triangles[i].material_id >= h.num_materials) { set_error("triangle material id out of range"); return DSRT_ERR_INVALID; }
    for (int i = 0; i < h.num_spheres; ++i) if (h.spheres[i].material_id < 0 || h.spheres[i].material_id >= h.num_materials) { set_error("sphere material id out of range"); return DSRT_ERR_INVALID; }

    PackArrays arr;
    std::vector<float4> mats;
    DeviceScene& v = out.view;
    std::memset(&v, 0, sizeof v);
    v.root_ref = kRefNone;
    v.accel_root_ref = kRefNone;
    out.has_second_tree = false;

    if (has_bvh) {
        const bool textured = h.num_textures > 0 && h.textures && h.texture_pool;
        arr.isect.reserve(((size_t)N / 2 + (size_t)M / 2 + 1) * 5 * (second_tree ? 2 : 1));
        arr.shade.reserve(((size_t)N + (size_t)M / 2 + 2) * 3 * (second_tree ? 2 : 1));
        PackedTree ref_tree, acc_tree;
        if (second_tree && N > 0) {
            // THE CERTIFIED SECOND TREE.  A ray's answer on the reference's tree is the accepted triangle of smallest t, except where it depends on the reference's own
            // boxes or order; path_machine.h checks, per ray, the three conditions under which it provably is (the certificate) and re-walks the reference tree
            // otherwise.  What the check needs from here: (a) the triangles the reference walk can never reach -- a zero-thickness box on their root-to-leaf path:
            // bbox_hit's `t_max <= t_min` holds with equality, src/gpu_render.cu:312 -- are left OUT of the second tree; (b) every triangle's leaf box ON THE
            // REFERENCE TREE rides with its slot (tri_cert); (c) the second tree's boxes are widened by 2^-16 of the scene's extent, so that no rounding of the slab
            // arithmetic makes a ray miss the box of a triangle it hits (ray origins up to 30 extents away: plan_render checks the camera).
            SecondTree st2;
            int rc = prepare_second_tree(h, second_tree_leaf_max(), st2);        // host/bvh_sah.cpp: unreachable triangles, reference-leaf boxes, the widened SAH tree, the checks
            if (rc != DSRT_OK) return rc;
            std::vector<GPUBVHNode>& nodes2 = st2.nodes;
            std::vector<int>& order2 = st2.order;
            std::vector<float>& leaf_box = st2.leaf_box;
            const GPUBVHNode& root = h.bvh_nodes[0];
            const float extent = st2.extent;
            const bool origins_near = st2.origins_near;
            // (both trees share one array of node records addressed by a 32-bit byte offset: a scene too big for two trees in it keeps the reference tree only)
            const bool fits = nodes2.size() / 2 + (size_t)M / 2 + 2 * (size_t)kRefBias < ((size_t)1 << 26) && (order2.size() + (size_t)N) / 2 + nodes2.size() / 2 + (size_t)M / 2 < ((size_t)1 << 28);
            if (!nodes2.empty() && origins_near && fits) {
                if ((rc = pack_tree(h, nodes2.data(), (int)nodes2.size(), order2.data(), (int)order2.size(), textured, leaf_box.data(), arr, acc_tree))) return rc;
                out.has_second_tree = true;
                out.scene_extent = extent;
                for (int a = 0; a < 3; ++a) out.scene_centre[a] = 0.5f * ((&root.bbox_min.x)[a] + (&root.bbox_max.x)[a]);
            }
        }
        int rc = pack_tree(h, h.bvh_nodes, M, h.tri_indices, N, textured, nullptr, arr, ref_tree, report);
        if (rc) return rc;
        for (int a = 0; a < 3; ++a) { v.root_lo[a] = ref_tree.lo[a]; v.root_hi[a] = ref_tree.hi[a]; v.accel_root_lo[a] = acc_tree.lo[a]; v.accel_root_hi[a] = acc_tree.hi[a]; }
        v.root_ref = ref_tree.root_ref;
        v.accel_root_ref = out.has_second_tree ? acc_tree.root_ref : kRefNone;
        v.stack_need = std::max(ref_tree.stack_need, acc_tree.stack_need);

        if (arr.isect.size() / 5 > (size_t)(1 << 28)) { set_error("too many triangle pair records"); return DSRT_ERR_INVALID; }
        if (arr.pairs.size() / 4 + kRefBias >= ((size_t)1 << 26)) { set_error("more than 2^26 - 64 internal BVH nodes (the kernel addresses node records by a 32-bit byte offset)"); return DSRT_ERR_INVALID; }
    }
    std::vector<float4>& pairs = arr.pairs; std::vector<float4>& isect = arr.isect; std::vector<float4>& shade = arr.shade; std::vector<float4>& uv = arr.uv;
    std::vector<int2>& big = arr.big; std::vector<int>& depth_of_all = arr.depth_of_all;
    mats.resize((size_t)h.num_materials * 3);
    for (int i = 0; i < h.num_materials; ++i) {
        const GPUMaterial& m = h.materials[i];
        mats[3 * (size_t)i + 0] = as_f4(bits(m.type), bits(m.albedo_tex), 0.0f, 0.0f);
        mats[3 * (size_t)i + 1] = as_f4(m.albedo.x, m.albedo.y, m.albedo.z, m.emissive.x);
        mats[3 * (size_t)i + 2] = as_f4(m.emissive.y, m.emissive.z, m.fuzz, m.ref_idx);
    }
    int num_lights = 0;                                                   // src/gpu_render.cu:841-847, a scene constant
    for (int i = 0; i < h.num_spheres; ++i) {
        const GPUMaterial& lm = h.materials[h.spheres[i].material_id];
        if (lm.type == MAT_DIFFUSE_LIGHT && (lm.emissive.x > 0 || lm.emissive.y > 0 || lm.emissive.z > 0)) num_lights++;
    }
    if (h.num_textures > 0 && h.textures && h.texture_pool) {
        for (int i = 0; i < h.num_textures; ++i) {
            const GPUTextureHeader& th = h.textures[i];
            if (th.width < 1 || th.height < 1 || th.offset < 0) { set_error("texture header out of range"); return DSRT_ERR_INVALID; }
        }
    }

    int rc;
    {
        std::vector<uint8_t> depth_bytes(pairs.size() / 4);
        for (size_t i = 0; i < depth_bytes.size(); ++i) depth_bytes[i] = (uint8_t)depth_of_all[i];
        if ((rc = out.pair_depth.upload(depth_bytes))) return rc;
    }
    if ((rc = out.pairs.upload(pairs)) || (rc = out.tri_pairs.upload(isect)) || (rc = out.tri_shade.upload(shade)) ||
        (rc = out.tri_uv.upload(uv)) || (rc = out.tri_cert.upload(arr.cert)) || (rc = out.big_leaves.upload(big)) || (rc = out.materials.upload(mats))) return rc;
    std::vector<GPUSphere> sph(h.spheres, h.spheres + h.num_spheres);
    if ((rc = out.spheres.upload(sph))) return rc;
    if (h.num_textures > 0 && h.textures && h.texture_pool) {
        std::vector<GPUTextureHeader> th(h.textures, h.textures + h.num_textures);
        std::vector<float> pool(h.texture_pool, h.texture_pool + h.texture_pool_floats);
        if ((rc = out.tex_headers.upload(th)) || (rc = out.tex_pool.upload(pool))) return rc;
    } else { out.tex_headers.reset(); out.tex_pool.reset(); }

    v.pair_depth = out.pair_depth.p; v.pairs = out.pairs.p; v.pairs_biased = reinterpret_cast<const char*>(reinterpret_cast<uintptr_t>(out.pairs.p) - (uintptr_t)kRefBias * 64u); v.tri_pairs = out.tri_pairs.p; v.tri_shade = out.tri_shade.p; v.tri_uv = out.tri_uv.p; v.tri_cert = out.tri_cert.p;
    v.big_leaves = out.big_leaves.p; v.materials = out.materials.p; v.spheres = out.spheres.p;
    v.tex_headers = out.tex_headers.p; v.tex_pool = out.tex_pool.p;
    v.num_pairs = (int)(pairs.size() / 4); v.num_tri_pairs = (int)(isect.size() / 5); v.num_big_leaves = (int)big.size();
    v.num_materials = h.num_materials; v.num_spheres = h.num_spheres; v.num_lights = num_lights;
    v.num_textures = (int)out.tex_headers.n; v.tex_pool_floats = (int)out.tex_pool.n;
    out.frame = frame_of(h);
    out.lean = h.num_spheres == 0 && out.tex_headers.n == 0;
    for (int i = 0; i < h.num_materials && out.lean; ++i) out.lean = h.materials[i].type == MAT_LAMBERTIAN;
    out.valid = true;
    return DSRT_OK;
}

}  // namespace

struct DsrtContext {
    int device = 0;
    int num_cus = 0;
    // The resident scene is shared between a context and its clones (dsrt_ctx_clone): one copy in HBM however many frames are in
    // flight.  Camera and sun are per context (they are what changes per frame); so are the working buffers below.
    std::shared_ptr<PackedScene> scene;
    FrameState frame;
    bool want_second_tree = false;  // dsrt_ctx_set_certified_tree / DSRT_CERTIFIED_TREE: the next upload also builds and packs the certified second tree
    DevBuf<uint32_t> ctrl;          // [0] queue, [1] flags, then counters (uint64 x kNumCounters) at byte 16
    DevBuf<uint2> spill;
    DevBuf<uint32_t> tile_cost, tile_order, tile_work, tile_tmp, probe_queue;
    DevBuf<BatchFrame> batch_table;  // dsrt_render_batch: one entry per frame
    std::vector<BatchFrame> batch_host;
    DevBuf<unsigned long long> accum_fixed;
    DevBuf<uint32_t> pixel_list;    // dsrt_render_accumulate_masked: the lists of active pixels (one entry per pixel of the shard's tiles)
    DevBuf<uint32_t> active_count;  // dsrt_select_unconverged: the word h_active is read from
    DevBuf<uint8_t> adaptive_mask;  // dsrt_render_adaptive: the mask between its passes
    DevBuf<uint32_t> gb_status;     // dsrt_render_gbuffer's status word
    DevBuf<uint32_t> rc_status;     // dsrt_trace_rays' status word
    DevBuf<float4> dn_cl[2], dn_vl[2], dn_nr, dn_xf, dn_al;   // dsrt_denoise_accumulated: 7 records of 16 bytes per pixel (launchers.h, DenoiseBuffers)
    DevBuf<float4> up_rec[5];       // dsrt_upscale_guided: 5 records of 16 bytes per LOW-resolution pixel (launchers.h, UpscaleRecords)
    // dsrt_render_denoised_temporal_to_host: the sequence the context keeps -- two histories (tp_hist[tp_cur] holds the last frame's), that frame's camera and size
    DevBuf<float4> tp_hist[2];
    GPUCamera tp_camera{};
    int tp_cur = 0, tp_width = 0, tp_height = 0;
    bool tp_valid = false;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t done = nullptr;      // recorded behind every render: the next render on ANY stream waits for it (queue words, spill strip,
    bool done_valid = false;        // pre-pass arrays and partial sums are per context, so a context has one render in flight)
    ~DsrtContext() { if (ev0) (void)hipEventDestroy(ev0); if (ev1) (void)hipEventDestroy(ev1); if (done) (void)hipEventDestroy(done); }
};

namespace {

// A fresh PackedScene for this context (clones made earlier keep the one they share until they are re-cloned or destroyed).
int build_bodies(const DsrtHostScene& hs, const PackReport& rep, PackedScene& sc);

// `bodies`: the host scene with the bodies tree that `host_layout` views (dsrt_scene_upload_bodies): no second tree, and the resident data of a pose update.
int install_scene(DsrtContext* ctx, const GPUScene& host_layout, const DsrtHostScene* bodies = nullptr) {
    auto fresh = std::make_shared<PackedScene>();
    ctx->scene.reset();
    PackReport report;
    int rc = pack_scene(host_layout, *fresh, ctx->want_second_tree && !bodies, bodies ? &report : nullptr);
    if (rc) return rc;
    if (bodies && (rc = build_bodies(*bodies, report, *fresh))) return rc;
    ctx->scene = std::move(fresh);
    ctx->frame = ctx->scene->frame;
    ctx->tp_valid = false;                         // a new scene: the temporal history of the old one is void
    return DSRT_OK;
}

static_assert(kMaxBodies == DSRT_MAX_BODIES, "launchers.h and include/dsrt.h disagree on the number of bodies");

// What a pose update needs resident, from the host scene's bodies tree and from where pack_tree put its nodes and triangles.
int build_bodies(const DsrtHostScene& hs, const PackReport& rep, PackedScene& sc) {
    auto bd = std::make_unique<BodiesResident>();
    const int B = (int)hs.body_start.size();
    const int M = (int)hs.nodes.size(), N = (int)hs.tris.size();
    bd->n_bodies = B;
    auto body_of_tri = [&](int t) { int b = 0; while (b + 1 < B && hs.body_start[b + 1] <= t) ++b; return b; };
    std::vector<int> node_body(M, -1), root_body_of(M, -1);                 // -1: a top node of the chain
    for (int b = 0; b < B; ++b) {
        if (hs.body_root[b] < 0) continue;
        root_body_of[hs.body_root[b]] = b;
        for (int i = 0; i < hs.body_nodes[b]; ++i) node_body[hs.body_root[b] + i] = b;
    }
    // movable entries, by body and then by pair record; the box of every pair record as the scene stands
    const size_t P = rep.pair_src.size();
    const int first_movable = B > 1 ? hs.body_start[1] : N;
    std::vector<std::vector<int>> by_body(B);
    std::vector<float4> box(2 * P);
    for (size_t pr = 0; pr < P; ++pr) {
        const int2 src = rep.pair_src[pr];
        float lo[3], hi[3];
        for (int w = 0; w < 2; ++w) {
            const int t = w ? src.y : src.x;
            if (t < 0) continue;
            const float* v = &hs.tris[t].v0.x;
            for (int k = 0; k < 3; ++k)
                for (int a = 0; a < 3; ++a) {
                    const float c = v[3 * k + a];
                    if (w == 0 && k == 0) lo[a] = hi[a] = c; else { lo[a] = fminf(lo[a], c); hi[a] = fmaxf(hi[a], c); }
                }
        }
        box[2 * pr] = as_f4(lo[0], lo[1], lo[2], 0.0f);
        box[2 * pr + 1] = as_f4(hi[0], hi[1], hi[2], 0.0f);
        const int b = body_of_tri(src.x);
        if (b >= 1) by_body[b].push_back((int)pr);
    }
    std::vector<float4> rest_v, rest_n;
    bd->entry_start.assign(B + 1, 0);
    for (int b = 1; b < B; ++b) {
        bd->entry_start[b] = (int)(rest_v.size() / 5);
        for (int pr : by_body[b]) {
            const int2 src = rep.pair_src[pr];
            float v[20] = {0}, nrm[20] = {0};
            for (int w = 0; w < 2; ++w) {
                const int t = w ? src.y : src.x;
                if (t < 0) continue;
                const float* r = &hs.rest[((size_t)t - first_movable) * 18];
                std::memcpy(v + 9 * w, r, 9 * sizeof(float));
                std::memcpy(nrm + 9 * w, r + 9, 9 * sizeof(float));
            }
            v[18] = bits(pr);
            v[19] = bits(b | (src.y >= 0 ? 256 : 0));
            for (int q = 0; q < 5; ++q) { rest_v.push_back(as_f4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3])); rest_n.push_back(as_f4(nrm[4 * q], nrm[4 * q + 1], nrm[4 * q + 2], nrm[4 * q + 3])); }
        }
    }
    bd->entry_start[B] = (int)(rest_v.size() / 5);
    if (B > 1) bd->entry_start[0] = bd->entry_start[1];
    // the internal records of the movable subtrees, deepest first; where the chain's nodes went
    std::vector<int> record_of(M, -1);
    int deepest = 0;
    for (size_t r = 0; r < rep.record_node.size(); ++r) { record_of[rep.record_node[r]] = (int)r; deepest = std::max(deepest, rep.record_depth[r]); }
    std::vector<int2> refit;
    for (int d = deepest; d >= 0; --d) {
        const int first = (int)refit.size();
        for (size_t r = 0; r < rep.record_node.size(); ++r)
            if (rep.record_depth[r] == d && node_body[rep.record_node[r]] >= 1) refit.push_back(make_int2((int)r, node_body[rep.record_node[r]]));
        if ((int)refit.size() > first) bd->depth_range.push_back(make_int2(first, (int)refit.size() - first));
    }
    std::vector<int4> chain;
    for (int c : hs.chain) {
        const GPUBVHNode& n = hs.nodes[c];
        chain.push_back(make_int4(record_of[c], root_body_of[n.left], std::max(root_body_of[n.right], 0), 0));
    }
    std::vector<float> pads(kMaxBodies, 0.0f), poses(kMaxBodies * 12, 0.0f);
    for (int b = 0; b < B; ++b) pads[b] = hs.body_pad[b];
    for (int b = 0; b < kMaxBodies; ++b) poses[12 * b] = poses[12 * b + 5] = poses[12 * b + 10] = 1.0f;
    int rc;
    if ((rc = bd->rest_v.upload(rest_v)) || (rc = bd->rest_n.upload(rest_n)) || (rc = bd->pair_box.upload(box)) || (rc = bd->poses.upload(poses)) || (rc = bd->pads.upload(pads)) ||
        (rc = bd->refit.upload(refit)) || (rc = bd->chain.upload(chain)) || (rc = bd->root_box.alloc(6))) return rc;
    for (hipEvent_t& e : bd->ev) HIP_TRY(hipEventCreate(&e));
    BodiesView& v = bd->view;
    v.pairs = sc.pairs.p; v.tri_pairs = sc.tri_pairs.p; v.tri_shade = sc.tri_shade.p; v.big_leaves = sc.big_leaves.p;
    v.rest_v = bd->rest_v.p; v.rest_n = bd->rest_n.p; v.pair_box = bd->pair_box.p; v.poses = bd->poses.p; v.pads = bd->pads.p;
    v.refit = bd->refit.p; v.chain = bd->chain.p; v.root_box = bd->root_box.p;
    v.n_chain = (int)chain.size();
    v.root_ref = sc.view.root_ref;
    v.root_body = 0;
    if (chain.empty()) for (int b = 0; b < B; ++b) if (hs.body_root[b] >= 0) v.root_body = b;
    v.num_pairs = sc.view.num_pairs; v.num_tri_pairs = sc.view.num_tri_pairs; v.num_big_leaves = sc.view.num_big_leaves;
    sc.bodies = std::move(bd);
    return DSRT_OK;
}

constexpr size_t kQueueLightWord = 96;                       // the light queue's counter: its own cache line, past the counters
constexpr size_t kCtrlWords = kQueueLightWord + 16;
constexpr size_t kListLenSched = 8;                          // masked accumulate launches: the lengths of the heavy and the light list (path_machine.h, LISTED) are words 8 and 9 of
                                                             // the pre-pass's sched block, next to the words every fetch reads anyway and away from the queue words' atomics
static_assert(4 + 2 * (size_t)kNumCounters <= kQueueLightWord, "counters overlap the second queue word");

float inv_gamma_of(const DsrtRenderDesc& d) { return 1.0f / (d.gamma > 0.0f ? d.gamma : 1.0f); }        // gamma <= 0 is 1, src/gpu_render.cu:1043

struct Tiling { int tile, tiles_x, tiles_y, total, mine, padded; };
bool make_tiling(const DsrtRenderDesc& d, Tiling& t) {
    t.tile = d.tile_size > 0 ? d.tile_size : 8;
    if (t.tile % 8 != 0 || t.tile > 1024 || d.width < 2 || d.height < 2) return false;
    const int count = d.shard_count > 1 ? d.shard_count : 1;
    if (d.shard_rank < 0 || d.shard_rank >= count) return false;
    t.tiles_x = (d.width + t.tile - 1) / t.tile;
    t.tiles_y = (d.height + t.tile - 1) / t.tile;
    t.total = t.tiles_x * t.tiles_y;
    t.mine = (t.total - d.shard_rank + count - 1) / count;
    t.padded = (t.total + count - 1) / count;
    return true;
}

// Development switches.  They are NOT part of a render's description (include/dsrt.h refuses unknown bits of DsrtRenderDesc.tune[3]); the A/B tools under
// tools/ set them through dsrt_dev_set_experiment(), and a process started with the environment variable DSRT_EXPERIMENT (an integer in C syntax) takes that as
// the initial word -- read ONCE, in the first dsrt_device_count / dsrt_ctx_create call, never per render.  Undefined bits are refused, and a non-zero word is
// announced on stderr, so that a stray variable cannot silently change how a production process schedules its work.
//   64           8 probe samples per pixel instead of 4
//   128          leaf records are not dealt to idle lanes (render_kernel.hip, phase L)
// (the low six bits are never used here: tools/ab_tune.py splits one number into the DSRT_TUNE_* flags and this word)
//   bits 8-19    rng_mode 1: slices per heavy pixel (0 = chosen by the pre-pass)
//   bits 20-22   grid = resident set >> n (frames that overlap on separate streams)
//   bit 24       the general kernels even for a scene that qualifies for the LEAN instantiation (A/B of the two)
//   bit 27       COUNTING BUILD of rng_mode 0 only: the float image receives per pixel (fetch time, end time, wave) as bit patterns,
//                100 MHz ticks, instead of the colour (tools/chain_timeline.py) -- the one switch that changes output (the float image; never the bytes)
//   bits 28-29   rng_mode 1: least samples per work item of a background pixel, 0 = 128, 1 = 64, 2 = 256, 3 = 512
//   bit 31       rng_mode 1: background pixels one item each
// Apart from bit 27 none of them changes a pixel (tests/test_gpu_parity.py runs the render under several of them against the oracle).
constexpr uint32_t kExperimentDefined = 64u | 128u | (0xFFFu << 8) | (7u << 20) | (1u << 24) | (1u << 27) | (3u << 28) | (1u << 31);
std::atomic<uint32_t> g_experiment{0u};

int set_experiment(uint32_t word, const char* from) {
    if (word & ~kExperimentDefined) {
        char buf[160];
        std::snprintf(buf, sizeof buf, "%s: development switch word 0x%x has undefined bits (defined: 0x%x)", from, word, kExperimentDefined);
        set_error(buf);
        return DSRT_ERR_INVALID;
    }
    if (word != g_experiment.exchange(word) && word) std::fprintf(stderr, "libdsrt_hip: development switches 0x%x in effect (%s)\n", word, from);
    return DSRT_OK;
}

void experiment_from_environment() {            // once per process
    static std::once_flag once;
    std::call_once(once, [] {
        const char* e = std::getenv("DSRT_EXPERIMENT");
        if (e && *e && set_experiment((uint32_t)std::strtoul(e, nullptr, 0), "environment variable DSRT_EXPERIMENT") != DSRT_OK)
            std::fprintf(stderr, "libdsrt_hip: DSRT_EXPERIMENT ignored: %s\n", dsrt_last_error());
    });
}

uint32_t experiment_word() { return g_experiment.load(); }

// The context's resident scene, or null ...
const PackedScene* scene_of(const DsrtContext* ctx) { return ctx && ctx->scene && ctx->scene->valid ? ctx->scene.get() : nullptr; }
// ... and for an entry point that needs one: null leaves "<fn>: no scene uploaded" as the error, and the caller returns DSRT_ERR_NO_SCENE.
const PackedScene* resident_scene(const DsrtContext* ctx, const char* fn) {
    const PackedScene* sc = scene_of(ctx);
    if (!sc) set_error(std::string(fn) + ": no scene uploaded");
    return sc;
}

// ONE LAUNCH AT A TIME PER CONTEXT.  A context's working buffers and status words serve one launch, so every entry point that launches goes through
//   launch_begin    the context's previous launch (on whatever stream it went) comes first; then this launch's device words are zeroed, in the order given
//   launch_clock    what is enqueued from here on is DsrtStats.kernel_ms (a pre-pass is enqueued before it)
//   launch_finish   `done` is recorded for the next launch to wait for; a caller that wants stats waits here and gets them zeroed but for kernel_ms
//   flags_result    the status word of a checked kernel, as a return code
struct Zeroed { void* p; size_t bytes; };
int launch_begin(DsrtContext* ctx, hipStream_t stream, std::initializer_list<Zeroed> zeroed) {
    if (ctx->done_valid) HIP_TRY(hipStreamWaitEvent(stream, ctx->done, 0));
    for (const Zeroed& z : zeroed) if (z.p) HIP_TRY(hipMemsetAsync(z.p, 0, z.bytes, stream));
    return DSRT_OK;
}
int launch_clock(DsrtContext* ctx, hipStream_t stream, const DsrtStats* stats) { if (stats) HIP_TRY(hipEventRecord(ctx->ev0, stream)); return DSRT_OK; }
int launch_finish(DsrtContext* ctx, hipStream_t stream, DsrtStats* stats) {
    HIP_TRY(hipEventRecord(ctx->done, stream));
    ctx->done_valid = true;
    if (!stats) return DSRT_OK;
    HIP_TRY(hipEventRecord(ctx->ev1, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    std::memset(stats, 0, sizeof *stats);
    HIP_TRY(hipEventElapsedTime(&stats->kernel_ms, ctx->ev0, ctx->ev1));
    return DSRT_OK;
}
int flags_result(const char* kernel, uint32_t flags) {
    if (!flags) return DSRT_OK;
    char buf[96];
    std::snprintf(buf, sizeof buf, "%s kernel raised status flags 0x%x", kernel, flags);
    set_error(buf);
    return DSRT_ERR_DEVICE_FLAG;
}
// All of it around a kernel without a pre-pass and with one status word of its own (the G-buffer pass, the ray queries).
template <typename Launch>
int launch_enveloped(DsrtContext* ctx, hipStream_t stream, uint32_t* status, DsrtStats* stats, const char* kernel, int waves, Launch&& launch) {
    int rc;
    if ((rc = launch_begin(ctx, stream, {{status, sizeof(uint32_t)}})) || (rc = launch_clock(ctx, stream, stats))) return rc;
    HIP_TRY(launch(stream));
    if ((rc = launch_finish(ctx, stream, stats)) || !stats) return rc;
    HIP_TRY(hipMemcpy(&stats->device_flags, status, sizeof(uint32_t), hipMemcpyDeviceToHost));
    stats->waves_launched = waves;
    return flags_result(kernel, stats->device_flags);
}

// STAGED HOST CALLS: the _to_host form of an entry point is its device form on device mirrors of the caller's host buffers.  A null host pointer (a channel
// not asked for) has no mirror; inputs are copied in before the call, results out after a successful one.
enum class Dir { In, Out, InOut };
struct Staged { const void* host; size_t bytes; Dir dir; };
template <size_t N, typename Call>
int staged_call(const Staged (&s)[N], Call&& call) {          // call(void* const* mirrors) -> return code
    DevBuf<uint8_t> mirror[N];
    void* dev[N] = {nullptr};
    for (size_t k = 0; k < N; ++k) {
        if (!s[k].host) continue;
        if (int rc = mirror[k].alloc(s[k].bytes)) return rc;
        dev[k] = mirror[k].p;
        if (dev[k] && s[k].dir != Dir::Out) HIP_TRY(hipMemcpy(dev[k], s[k].host, s[k].bytes, hipMemcpyHostToDevice));
    }
    if (int rc = call(dev)) return rc;
    for (size_t k = 0; k < N; ++k)
        if (dev[k] && s[k].dir != Dir::In) HIP_TRY(hipMemcpy(const_cast<void*>(s[k].host), dev[k], s[k].bytes, hipMemcpyDeviceToHost));
    return DSRT_OK;
}

// Bytes per element of the channels of include/dsrt.h's structs of pointers, in the order of their members.
constexpr size_t kRayBytes[4] = {12, 12, 4, 4};                                // DsrtRays: origins, dirs, t_min, t_max
constexpr size_t kRayHitBytes[9] = {4, 4, 12, 12, 8, 12, 4, 4, 1};             // DsrtRayHits: t, range, position, normal, uv, albedo, prim_id, material_id, flags
constexpr size_t kGBufferBytes[11] = {4, 4, 4, 12, 12, 8, 12, 4, 4, 4, 1};     // DsrtGBuffer: t, range, depth, position, normal, uv, albedo, prim_id, material_id, sun_cos, flags
static_assert(sizeof(DsrtRays) == 4 * sizeof(void*), "kRayBytes has one entry per pointer of DsrtRays");
static_assert(sizeof(DsrtRayHits) == 9 * sizeof(void*), "kRayHitBytes has one entry per pointer of DsrtRayHits");
static_assert(sizeof(DsrtGBuffer) == 11 * sizeof(void*), "kGBufferBytes has one entry per pointer of DsrtGBuffer");
constexpr int kRayHitFlags = 8;                                               // `flags` in kRayHitBytes: the one channel DSRT_TRACE_ANY writes
static_assert(offsetof(DsrtRayHits, flags) == kRayHitFlags * sizeof(void*) && kRayHitBytes[kRayHitFlags] == 1, "kRayHitFlags is the place of DsrtRayHits.flags");
static_assert(sizeof(DsrtAccum) == 2 * sizeof(void*), "DsrtAccum is {sum, sum_sq}: the first two mirrors of the accumulate and resolve host forms");

// Such a struct's channels of `n` elements each as Staged entries, and the struct again from the mirrors of those entries.
template <typename S, size_t N>
void channels(const S& s, const size_t (&bytes_per)[N], size_t n, Dir dir, Staged* out) {
    static_assert(sizeof(S) == N * sizeof(void*), "one table entry per pointer of the struct");
    const void* p[N];
    std::memcpy(p, &s, sizeof p);
    for (size_t k = 0; k < N; ++k) out[k] = Staged{p[k], n * bytes_per[k], dir};
}
template <typename S>
S pointers_as(void* const* mirrors) {              // the caller's list has sizeof(S) / sizeof(void*) entries from `mirrors` on, in S's order
    static_assert(std::is_trivially_copyable_v<S> && sizeof(S) % sizeof(void*) == 0, "a struct of pointers and nothing else");
    S s; std::memcpy(&s, mirrors, sizeof s); return s;
}

// A SAMPLE-SET FRAME'S BUFFERS, once: the sums and counts, the denoiser's guides, the image outputs and the temporal stage's four, each with its bytes per pixel, its
// direction and the alignment its kernel needs.  check_denoise walks the table; the _to_host forms stage it (staged_frame_call).  A form leaves what it does not take null.
// The upscaler (dsrt_upscale_guided) has two rasters: the rows above are then the OUTPUT resolution's (its guides and images), and its own rows hold what it reads and
// writes at the LOW resolution (`lo` in the table: that raster's pixel count sizes them), the output raster's flags and the support.
struct FrameBuffers {
    const void *sum, *sum_sq, *n;                                      // DsrtAccum, then the per-pixel counts
    const void *normal, *position, *albedo, *range;                    // DsrtDenoiseGuides
    const void *rgb8, *f32, *linear, *var;                             // the image outputs
    const void *history_prev, *history_next, *prev_xy, *weight;        // the temporal stage's
    const void *lo_linear, *lo_var, *lo_normal, *lo_position, *lo_albedo, *lo_range, *lo_flags, *lo_rgb8;      // the upscaler's, low resolution ...
    const void *flags, *support;                                       // ... and output resolution
};
struct FrameBufferKind { size_t bytes; Dir dir; size_t align; bool lo = false; };
constexpr size_t kHistoryBytes = 64;                                   // per pixel: include/dsrt.h, TEMPORAL ACCUMULATION
constexpr FrameBufferKind kFrameBuffers[] = {
    {24, Dir::In, 8}, {24, Dir::In, 8}, {4, Dir::In, 4},                                                  // (bytes per pixel, direction, alignment) in FrameBuffers' order,
    {12, Dir::In, 4}, {12, Dir::In, 4}, {12, Dir::In, 4}, {4, Dir::In, 4},                                // a row of this table per row of the struct
    {3, Dir::Out, 1}, {12, Dir::Out, 4}, {12, Dir::Out, 4}, {12, Dir::Out, 4},
    {kHistoryBytes, Dir::In, 16}, {kHistoryBytes, Dir::Out, 16}, {8, Dir::Out, 4}, {4, Dir::Out, 4},
    {12, Dir::In, 4, true}, {12, Dir::In, 4, true}, {12, Dir::In, 4, true}, {12, Dir::In, 4, true}, {12, Dir::In, 4, true}, {4, Dir::In, 4, true}, {1, Dir::In, 1, true},
    {3, Dir::Out, 1, true}, {1, Dir::In, 1}, {4, Dir::Out, 4}};
constexpr size_t kFrameBufferCount = sizeof(FrameBuffers) / sizeof(void*);
constexpr size_t kFrameTemporal = offsetof(FrameBuffers, history_prev) / sizeof(void*);
constexpr size_t kFrameUpscale = offsetof(FrameBuffers, lo_linear) / sizeof(void*);
static_assert(sizeof kFrameBuffers / sizeof kFrameBuffers[0] == kFrameBufferCount, "kFrameBuffers has one entry per pointer of FrameBuffers");

void frame_table(const FrameBuffers& b, size_t px, Staged (&s)[kFrameBufferCount], size_t px_lo = 0) {
    const void* p[kFrameBufferCount];
    std::memcpy(p, &b, sizeof p);
    for (size_t k = 0; k < kFrameBufferCount; ++k) s[k] = Staged{p[k], (kFrameBuffers[k].lo ? px_lo : px) * kFrameBuffers[k].bytes, kFrameBuffers[k].dir};
}
DsrtAccum accum_of(const FrameBuffers& b) { return DsrtAccum{(uint64_t*)b.sum, (uint64_t*)b.sum_sq}; }

// staged_call over a frame's table: call(the mirrors, by name) -> return code.  `finish`: the device has finished before the results are copied out.
template <typename Call>
int staged_frame_call(const FrameBuffers& host, size_t px, bool finish, Call&& call, size_t px_lo = 0) {
    Staged s[kFrameBufferCount];
    frame_table(host, px, s, px_lo);
    return staged_call(s, [&](void* const* d) -> int {
        if (int rc = call(pointers_as<FrameBuffers>(d))) return rc;
        if (finish) HIP_TRY(hipStreamSynchronize(nullptr));
        return DSRT_OK;
    });
}

// Ray queries (raycast_kernel.hip).  Argument checks shared by the device and the host form: every range is known from `count`.
bool ranges_overlap(const Staged& a, const Staged& b) {
    if (!a.host || !b.host || !a.bytes || !b.bytes) return false;
    const uintptr_t a0 = (uintptr_t)a.host, b0 = (uintptr_t)b.host;
    return a0 < b0 + b.bytes && b0 < a0 + a.bytes;
}

int check_trace_args(const char* fn, const DsrtContext* ctx, int count, const DsrtRays* rays, int mode, const DsrtRayHits* hits) {
    auto fail = [&](const char* why) { set_error(std::string(fn) + ": " + why); return DSRT_ERR_INVALID; };
    if (!ctx || !rays || !hits) return fail("null argument");
    if (!rays->origins || !rays->dirs) return fail("null origins or dirs");
    if (count < 0) return fail("count < 0");
    if (mode != DSRT_TRACE_CLOSEST && mode != DSRT_TRACE_ANY) return fail("unknown mode");
    Staged in[4], out[9];
    channels(*rays, kRayBytes, (size_t)count, Dir::In, in);
    channels(*hits, kRayHitBytes, (size_t)count, Dir::Out, out);
    bool any_out = false, non_flag_out = false;
    for (int k = 0; k < 9; ++k) if (out[k].host) { any_out = true; if (k != kRayHitFlags) non_flag_out = true; }
    if (!any_out) return fail("no output channel");
    if (mode == DSRT_TRACE_ANY && non_flag_out) return fail("DSRT_TRACE_ANY writes `flags` only");
    for (const Staged& r : in) if ((uintptr_t)r.host & 3u) return fail("pointer not 4-byte aligned");
    for (const Staged& r : out) if ((uintptr_t)r.host & 3u) return fail("pointer not 4-byte aligned");
    for (const Staged& o : out)
        for (const Staged& i : in)
            if (ranges_overlap(o, i)) return fail("an output range overlaps an input range");
    return DSRT_OK;
}

// GPUScene's seven arrays, each as f(pointer, elements): `elements` is the array's count where the pointer is set and 0 where it is null; tri_indices has no count
// of its own but one entry per triangle, and bvh_tri_indices is its alias (include/dsrt_scene_abi.h).  f may replace the pointer; the first non-zero return ends the walk.
constexpr size_t kSceneArrays = 7;                 // calls of f per walk (what a caller keeps per array is sized by this)
template <typename Scene, typename F>
int for_each_scene_array(Scene& s, F&& f) {
    auto elements = [](const void* p, int count) { return p ? (size_t)count : (size_t)0; };
    int rc;
    if ((rc = f(s.triangles, elements(s.triangles, s.num_triangles))) || (rc = f(s.spheres, elements(s.spheres, s.num_spheres))) ||
        (rc = f(s.materials, elements(s.materials, s.num_materials))) || (rc = f(s.tri_indices, elements(s.tri_indices, s.num_triangles)))) return rc;
    if constexpr (!std::is_const_v<Scene>) s.bvh_tri_indices = const_cast<int*>(s.tri_indices);
    if ((rc = f(s.bvh_nodes, elements(s.bvh_nodes, s.num_bvh_nodes))) || (rc = f(s.textures, elements(s.textures, s.num_textures))) ||
        (rc = f(s.texture_pool, elements(s.texture_pool, s.texture_pool_floats)))) return rc;
    return DSRT_OK;
}

}  // namespace

extern "C" {

int dsrt_dev_set_experiment(uint32_t word) {
    experiment_from_environment();              // (so that a later first context does not overwrite this call's word with the variable's)
    return set_experiment(word, "dsrt_dev_set_experiment");
}

int dsrt_device_count(void) {
    hw_queues_default();
    experiment_from_environment();
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int dsrt_ctx_create(int device, DsrtContext** out) {
    if (!out) { set_error("dsrt_ctx_create: null out"); return DSRT_ERR_INVALID; }
    *out = nullptr;
    hw_queues_default();
    experiment_from_environment();
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { set_error("no HIP device visible"); return DSRT_ERR_NO_DEVICE; }
    if (device < 0 || device >= n) { set_error("device index out of range"); return DSRT_ERR_INVALID; }
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_error(std::string("device is ") + prop.gcnArchName + ", this library carries gfx950 code only");
        return DSRT_ERR_NO_DEVICE;
    }
    auto* ctx = new DsrtContext();
    ctx->device = device;
    ctx->num_cus = prop.multiProcessorCount;
    if (const char* e = std::getenv("DSRT_CERTIFIED_TREE")) ctx->want_second_tree = e[0] == '1';
    int rc = ctx->ctrl.alloc(kCtrlWords);
    if (rc) { delete ctx; return rc; }
    if (!hip_ok(hipEventCreate(&ctx->ev0), "hipEventCreate") || !hip_ok(hipEventCreate(&ctx->ev1), "hipEventCreate") ||
        !hip_ok(hipEventCreateWithFlags(&ctx->done, hipEventDisableTiming), "hipEventCreateWithFlags")) { delete ctx; return DSRT_ERR_HIP; }
    *out = ctx;
    return DSRT_OK;
}

int dsrt_ctx_clone(const DsrtContext* src, DsrtContext** out) {
    if (!src || !out) { set_error("dsrt_ctx_clone: null argument"); return DSRT_ERR_INVALID; }
    const int rc = dsrt_ctx_create(src->device, out);
    if (rc) return rc;
    (*out)->scene = src->scene;                    // shared, read-only on the device
    (*out)->want_second_tree = src->want_second_tree;
    (*out)->frame = src->frame;
    return DSRT_OK;
}

int dsrt_ctx_device(const DsrtContext* ctx) { return ctx ? ctx->device : -1; }

int dsrt_ctx_set_certified_tree(DsrtContext* ctx, int on) {
    if (!ctx) { set_error("dsrt_ctx_set_certified_tree: null context"); return DSRT_ERR_INVALID; }
    ctx->want_second_tree = on != 0;
    return DSRT_OK;
}

int dsrt_ctx_has_certified_tree(const DsrtContext* ctx) { const PackedScene* sc = scene_of(ctx); return sc && sc->has_second_tree ? 1 : 0; }

void dsrt_ctx_destroy(DsrtContext* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    delete ctx;
}

int dsrt_scene_upload(DsrtContext* ctx, const GPUScene* scene) {
    return dsrt::guarded("dsrt_scene_upload", [&]() -> int {
    if (!ctx || !scene) { set_error("dsrt_scene_upload: null argument"); return DSRT_ERR_INVALID; }
    HIP_TRY(hipSetDevice(ctx->device));
    return install_scene(ctx, *scene);
    });
}

int dsrt_scene_upload_device(DsrtContext* ctx, const GPUScene* d) {
    return dsrt::guarded("dsrt_scene_upload_device", [&]() -> int {
    if (!ctx || !d) { set_error("dsrt_scene_upload_device: null argument"); return DSRT_ERR_INVALID; }
    HIP_TRY(hipSetDevice(ctx->device));
    if (d->num_triangles < 0 || d->num_spheres < 0 || d->num_materials < 0 || d->num_bvh_nodes < 0 || d->num_textures < 0 || d->texture_pool_floats < 0) {
        set_error("scene has a negative count"); return DSRT_ERR_INVALID;
    }
    // Bring the reference-layout arrays back to the host, then convert as usual.
    GPUScene h = *d;
    std::vector<uint8_t> host[kSceneArrays];                          // (bytes from operator new: aligned for every element type of the scene)
    size_t k = 0;
    const int rc = for_each_scene_array(h, [&](auto*& p, size_t n) -> int {
        assert(k < kSceneArrays);
        std::vector<uint8_t>& to = host[k++];
        to.resize(n * sizeof(*p));
        if (n) HIP_TRY(hipMemcpy(to.data(), p, to.size(), hipMemcpyDeviceToHost));
        p = n ? reinterpret_cast<std::remove_reference_t<decltype(p)>>(to.data()) : nullptr;
        return DSRT_OK;
    });
    if (rc) return rc;
    return install_scene(ctx, h);
    });
}

int dsrt_scene_set_camera_sun(DsrtContext* ctx, const GPUCamera* cam, const float sun_dir_model[3]) {
    if (!ctx || !cam) { set_error("dsrt_scene_set_camera_sun: null argument"); return DSRT_ERR_INVALID; }
    if (!resident_scene(ctx, "dsrt_scene_set_camera_sun")) return DSRT_ERR_NO_SCENE;
    ctx->frame.camera = *cam;
    if (sun_dir_model) ctx->frame.sun_dir = DsrtF3{sun_dir_model[0], sun_dir_model[1], sun_dir_model[2]};
    return DSRT_OK;
}

int dsrt_scene_upload_bodies(DsrtContext* ctx, const DsrtHostScene* hs, const GPUScene* frame) {
    return dsrt::guarded("dsrt_scene_upload_bodies", [&]() -> int {
    if (!ctx || !hs || !frame) { set_error("dsrt_scene_upload_bodies: null argument"); return DSRT_ERR_INVALID; }
    if (!hs->bvh_valid || !hs->bodies_tree) { set_error("dsrt_scene_upload_bodies: the scene's tree is not the bodies tree (dsrt_host_scene_build_bvh_bodies)"); return DSRT_ERR_INVALID; }
    GPUScene s = *frame, g;                        // camera, params, Sun (and sky, seed) from `frame`, every array from the host scene
    int rc = dsrt_host_scene_view(hs, &g);
    if (rc) return rc;
    s.spheres = g.spheres; s.num_spheres = g.num_spheres;
    s.triangles = g.triangles; s.tri_indices = g.tri_indices; s.num_triangles = g.num_triangles;
    s.bvh_nodes = g.bvh_nodes; s.num_bvh_nodes = g.num_bvh_nodes; s.bvh_tri_indices = g.bvh_tri_indices;
    s.materials = g.materials; s.num_materials = g.num_materials;
    s.textures = g.textures; s.num_textures = g.num_textures;
    s.texture_pool = g.texture_pool; s.texture_pool_floats = g.texture_pool_floats;
    HIP_TRY(hipSetDevice(ctx->device));
    return install_scene(ctx, s, hs);
    });
}

int dsrt_ctx_body_count(const DsrtContext* ctx) { const PackedScene* sc = scene_of(ctx); return sc && sc->bodies ? sc->bodies->n_bodies : 0; }

int dsrt_ctx_body_update_ms(const DsrtContext* ctx, float ms[3]) {
    const PackedScene* sc = scene_of(ctx);
    if (!sc || !sc->bodies || !ms) { set_error("dsrt_ctx_body_update_ms: no scene with bodies, or null argument"); return DSRT_ERR_INVALID; }
    for (int i = 0; i < 3; ++i) ms[i] = sc->bodies->last_ms[i];
    return DSRT_OK;
}

int dsrt_scene_set_body_poses(DsrtContext* ctx, int first_body, int count, const float* poses, void* stream_v, float* ms) {
    if (!ctx) { set_error("dsrt_scene_set_body_poses: null context"); return DSRT_ERR_INVALID; }
    if (!resident_scene(ctx, "dsrt_scene_set_body_poses")) return DSRT_ERR_NO_SCENE;
    PackedScene& sc = *ctx->scene;
    if (!sc.bodies) { set_error("dsrt_scene_set_body_poses: the resident scene has no bodies (dsrt_scene_upload_bodies)"); return DSRT_ERR_INVALID; }
    BodiesResident& bd = *sc.bodies;
    const int rc = check_body_poses(bd.n_bodies, first_body, count, poses, "dsrt_scene_set_body_poses");
    if (rc) return rc;
    if (ms) *ms = 0.0f;
    if (!count) return DSRT_OK;
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    HIP_TRY(hipSetDevice(ctx->device));
    if (ctx->done_valid) HIP_TRY(hipStreamWaitEvent(stream, ctx->done, 0));
    HIP_TRY(hipMemcpyAsync(bd.poses.p + 12 * (size_t)first_body, poses, 12 * (size_t)count * sizeof(float), hipMemcpyHostToDevice, stream));
    if (ms) HIP_TRY(hipEventRecord(bd.ev[0], stream));
    const int e0 = bd.entry_start[first_body], e1 = bd.entry_start[first_body + count];
    HIP_TRY(launch_bodies_transform(bd.view, e0, e1 - e0, stream));
    if (ms) HIP_TRY(hipEventRecord(bd.ev[1], stream));
    for (const int2& r : bd.depth_range) HIP_TRY(launch_bodies_refit(bd.view, r.x, r.y, stream));
    if (ms) HIP_TRY(hipEventRecord(bd.ev[2], stream));
    HIP_TRY(launch_bodies_chain(bd.view, stream));
    if (ms) HIP_TRY(hipEventRecord(bd.ev[3], stream));
    float root[6];
    HIP_TRY(hipMemcpyAsync(root, bd.root_box.p, sizeof root, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    for (int a = 0; a < 3; ++a) { sc.view.root_lo[a] = root[a]; sc.view.root_hi[a] = root[3 + a]; }
    ctx->tp_valid = false;                         // the temporal history assumed the scene as it was
    if (ms) {
        for (int i = 0; i < 3; ++i) HIP_TRY(hipEventElapsedTime(&bd.last_ms[i], bd.ev[i], bd.ev[i + 1]));
        HIP_TRY(hipEventElapsedTime(ms, bd.ev[0], bd.ev[3]));
    }
    return DSRT_OK;
}

int dsrt_shard_layout(const DsrtRenderDesc* desc, int* tiles_total, int* tiles_this_shard, int* tiles_per_shard_padded, size_t* rgb8_bytes_padded) {
    Tiling t;
    if (!desc || !make_tiling(*desc, t)) { set_error("dsrt_shard_layout: bad descriptor"); return DSRT_ERR_INVALID; }
    if (tiles_total) *tiles_total = t.total;
    if (tiles_this_shard) *tiles_this_shard = t.mine;
    if (tiles_per_shard_padded) *tiles_per_shard_padded = t.padded;
    if (rgb8_bytes_padded) *rgb8_bytes_padded = (size_t)t.padded * t.tile * t.tile * 3;
    return DSRT_OK;
}

// What a batch launch adds to a render: the frames' cameras and sun directions (the context's own camera is not used).
struct BatchInput { int frames; const GPUCamera* cameras; const DsrtF3* sun_dirs; };
// What an accumulate launch changes (dsrt_render_accumulate, checked there): the samples rendered -- {first + j*stride : 0 <= j < count} of a frame
// planned at desc->spp -- and where their sums go (the caller's buffers, added to, never cleared; no resolve).
// mask (dsrt_render_accumulate_masked; null = every pixel): only the pixels whose byte is set; n (optional): their sample counts, `count` added.
struct AccumInput { int first, count, stride; unsigned long long* sum; unsigned long long* sum_sq; const uint8_t* mask; uint32_t* n; };

// ---- A render launch (dsrt_render, dsrt_render_batch, dsrt_render_accumulate), in stages: plan_render refuses or decides everything, without a HIP call;
// grow_render_buffers sizes the context's working buffers; one of the three pre-passes orders the tiles; launch_and_resolve; read_render_stats. ----
namespace {

constexpr int kLdsStackEntries = 8;                      // LDS short-stack: 8 entries per lane (what fits beside the tree top and the continuation strip); deeper entries spill.
constexpr int kThreadsPerBlock = 64 * kWavesPerBlock;
constexpr int kProbeSpp = 4;          // x every pixel of the heavy tiles: 7 ms at 1080p, near frame.  (1, 2, 4 or 8 samples order the tiles equally well.)

enum class PrePass { Batch, Ordered, Natural };

struct RenderPlan {
    Tiling t;
    RenderArgs a;                     // complete but for what grow_render_buffers (accum_fixed of the context's own sums, spill, sched) and the pre-pass (tile order, batch table) add
    RenderVariant variant;
    const RenderLaunchers* rl;
    PrePass pre;
    bool cull, probe;                 // the pre-pass removes provably empty tiles / re-sorts the heavy tiles by measured cost ...
    int probe_spp;                    // ... at this many samples per pixel
    bool own_sums;                    // rng_mode 1 of dsrt_render(_batch): the sums are the context's, zeroed before and resolved behind the launch
    int frames, chunks, chunk_len, blocks;
    size_t out_pixels, pre_stride;    // pre_stride, per frame: tile costs / order, then the sched words
    uint32_t* sched;                  // {tiles that see geometry, tiles in the order, heavy lanes per wave}: the words 32 entries past the cost array (grow_render_buffers)
};

}  // namespace

static int plan_render(const DsrtContext* ctx, const DsrtRenderDesc* desc, uint8_t* d_rgb8, float* d_f32, const BatchInput* batch, const AccumInput* acc, RenderPlan& p) {
    if (!ctx || !desc || (!d_rgb8 && !acc)) { set_error("dsrt_render: null argument"); return DSRT_ERR_INVALID; }
    const PackedScene* scp = resident_scene(ctx, "dsrt_render");
    if (!scp) return DSRT_ERR_NO_SCENE;
    const PackedScene& sc = *scp;
    if (desc->rng_mode != 0 && desc->rng_mode != 1) { set_error("dsrt_render: rng_mode must be 0 (reference LCG stream per pixel) or 1 (Philox4x32-10 stream per sample)"); return DSRT_ERR_INVALID; }
    if (desc->math_mode != 0 && desc->math_mode != 1) { set_error("dsrt_render: math_mode must be 0 (deterministic sin / cos / pow shared with the CPU oracle) or 1 (the device math library's)"); return DSRT_ERR_INVALID; }
    p.rl = &render_launchers(desc->math_mode == 1);
    if (desc->tune[3] & ~DSRT_TUNE_FLAG_MASK) { set_error("dsrt_render: tune[3] has bits set that this ABI version does not define (DSRT_TUNE_* in include/dsrt.h)"); return DSRT_ERR_INVALID; }
    const uint32_t flags = (uint32_t)desc->tune[3];
    const uint32_t xp = experiment_word();
    const bool lean = sc.lean && !(xp & (1u << 24));
    Tiling& t = p.t;
    if (!make_tiling(*desc, t)) { set_error("dsrt_render: bad size, tile or shard"); return DSRT_ERR_INVALID; }

    RenderArgs& a = p.a;
    std::memset(&a, 0, sizeof a);
    a.scene = sc.view;
    FrameParams& f = a.frame;
    const FrameState& fs = ctx->frame;
    pack_camera(fs.camera, f.cam);
    f.sun_dir[0] = fs.sun_dir.x; f.sun_dir[1] = fs.sun_dir.y; f.sun_dir[2] = fs.sun_dir.z;
    f.sun_radiance[0] = fs.sun_radiance.x; f.sun_radiance[1] = fs.sun_radiance.y; f.sun_radiance[2] = fs.sun_radiance.z;
    f.sun_enabled = fs.sun_enabled;
    f.width = desc->width; f.height = desc->height;
    f.plan_spp = desc->spp < 1 ? 1 : desc->spp;                         // src/gpu_render.cu:987-988
    f.spp = acc ? acc->count : f.plan_spp;                               // what the launch renders of each pixel: work items, slices and the pre-pass count these
    f.sample_first = acc ? acc->first : 0;
    f.sample_stride = acc ? acc->stride : 1;
    f.max_depth = desc->max_depth > 0 ? desc->max_depth : 12;           // :723-725
    f.inv_gamma = inv_gamma_of(*desc);
    f.seed32 = (uint32_t)(desc->seed & 0xFFFFFFFFu);
    f.seed_hi = (uint32_t)(desc->seed >> 32);
    f.tile = t.tile; f.tiles_x = t.tiles_x; f.tiles_y = t.tiles_y;
    f.shard_rank = desc->shard_rank; f.shard_count = desc->shard_count > 1 ? desc->shard_count : 1;
    f.local_tiles = t.mine;
    if ((unsigned long long)t.mine * (unsigned long long)(t.tile * t.tile) >= (1ull << 31)) { set_error("dsrt_render: image too large (2^31 pixels per shard)"); return DSRT_ERR_INVALID; }
    uint32_t total_items = (uint32_t)t.mine * (uint32_t)(t.tile * t.tile);
    f.compact_output = desc->shard_count > 1 ? 1 : 0;
    p.chunks = 1; p.chunk_len = f.spp;
    f.light_chunk_len = f.spp;
    p.frames = batch ? batch->frames : 1;
    if (batch) {
        if (p.frames < 1 || !batch->cameras || !batch->sun_dirs) { set_error("dsrt_render_batch: no frames"); return DSRT_ERR_INVALID; }
        if (desc->collect_counters || desc->checked) { set_error("dsrt_render_batch uses the production kernel only (no counters, not checked)"); return DSRT_ERR_INVALID; }
        // 32-bit output indices and work-item numbers: frames x pixels (x 8 sample slices in rng_mode 1) stay below 2^32
        const unsigned long long frame_px = desc->shard_count > 1 ? (unsigned long long)t.padded * t.tile * t.tile : (unsigned long long)desc->width * desc->height;
        if ((unsigned long long)p.frames * frame_px * (desc->rng_mode == 1 ? 16ull : 1ull) >= (1ull << 32)) {
            set_error("dsrt_render_batch: too many pixels in one batch (split the sequence)"); return DSRT_ERR_INVALID;
        }
    }
    p.out_pixels = (desc->shard_count > 1 ? (size_t)t.padded * t.tile * t.tile : (size_t)desc->width * desc->height) * (size_t)p.frames;
    p.own_sums = desc->rng_mode == 1 && !acc;
    if (desc->rng_mode == 1) {
        // a pixel's samples are independent streams: pixels of tiles that see geometry are split into 8 work items.  More slices cost
        // more in half-empty advance passes than their shorter tail saves; fewer leave whole waves without work at the end of a small
        // job, which sample stealing (inside a wave, path_machine.h) cannot repair.  One rank's share of an 8-GPU 1080p x 1000 frame,
        // stealing on: 1 / 2 / 4 / 8 / 16 / 32 / 64 slices = 307 / 289 / 188 / 171 / 181 / 191 / 203 ms; whole frame on one GPU
        // 1091 / 1076 / 1063 / 1050 / 1047 (profiles/r02/README.md).  An item's integer sums are 32-bit in units of 2^-20: at most 4095
        // samples per item, so with more samples than that every pixel is sliced, whatever its tile sees.
        int chunk_len = (f.spp + 7) / 8;
        if ((xp >> 8) & 0xFFFu) chunk_len = (f.spp + (int)((xp >> 8) & 0xFFFu) - 1) / (int)((xp >> 8) & 0xFFFu);   // experiment: slices per pixel
        // Sample sets: a set of few samples per pixel (one of many interleaved passes) is not cut below kSetMinItem samples per item.  One of ten passes
        // of the 1080p x 1000 near frame (100 samples): 8 slices of 13 = 114.6 ms, 4 / 2 / 1 slices = 87 / 86 / 88 ms; passes of 250 samples: 189 ms with 8
        // slices, 190-198 with fewer (slices forced by development switch bits 8-19).  dsrt_render keeps its own cut.
        constexpr int kSetMinItem = 32;
        if (acc && !((xp >> 8) & 0xFFFu)) chunk_len = std::max(chunk_len, std::min(f.spp, kSetMinItem));
        if (chunk_len < 1) chunk_len = 1;
        if (chunk_len > 4095) chunk_len = 4095;
        p.chunk_len = chunk_len;
        p.chunks = (f.spp + chunk_len - 1) / chunk_len;
        // Background pixels (tiles that see no geometry) are cut too, but not below kLightLen samples per item: uncut, their 1000-sample
        // items are the longest jobs of a frame and the light queue is served last (one of 8 shares of the near frame 166 -> 149 ms, frame
        // 70 60 -> 43 ms); cut as finely as the heavy pixels, their three 64-bit atomics per item cost the 250-spp sequence, whose frames
        // overlap and have no tail to lose, a fifth of its frame rate (47 -> 38 frames/s).
        {
            const int code = (int)((xp >> 28) & 3u);                                          // experiment
            const int kLightLen = code == 0 ? 128 : (code == 1 ? 64 : (code == 2 ? 256 : 512));
            f.light_chunk_len = (xp & 0x80000000u) ? f.spp : std::max(chunk_len, kLightLen);
            if (f.light_chunk_len > 4095) f.light_chunk_len = 4095;
        }
        if (desc->width > 65535 || desc->height > 65535) { set_error("dsrt_render: rng_mode 1 hands samples between lanes with 16-bit pixel coordinates (width, height <= 65535)"); return DSRT_ERR_INVALID; }
        if ((unsigned long long)total_items * 64ull >= (1ull << 32)) { set_error("dsrt_render: image too large for rng_mode 1 (more than 2^32 sample slices)"); return DSRT_ERR_INVALID; }
        total_items *= 64u;                                     // upper bound (the pre-pass picks 8 to 64 slices per heavy pixel): sizes the grid only
        if (acc) {                                              // the caller's sums, added to (the context's own: grow_render_buffers; 24 bytes per pixel)
            a.accum_fixed = acc->sum;
            a.accum_sq = acc->sum_sq;
        }
    }
    a.out_rgb8 = d_rgb8;
    a.out_f32 = d_f32;
    a.queue = ctx->ctrl.p;
    a.queue_light = ctx->ctrl.p + kQueueLightWord;
    a.flags = ctx->ctrl.p + 1;
    a.counters = (uint64_t*)(ctx->ctrl.p + 4);

    if (desc->stack_entries != 0 && desc->stack_entries != kLdsStackEntries) { set_error("dsrt_render: stack_entries must be 0 or 8"); return DSRT_ERR_INVALID; }
    const int resident_blocks = ctx->num_cus * 4;                         // 4 waves per SIMD = 4 workgroups of 4 waves per CU (render_kernel.hip)
    p.blocks = resident_blocks;                                           // persistent: exactly the resident set
    if ((xp >> 20) & 7u) p.blocks = std::max(1, resident_blocks >> ((xp >> 20) & 7u));     // experiment: a fraction of it (frames that overlap)
    {
        const long long needed = ((long long)total_items + kThreadsPerBlock - 1) / kThreadsPerBlock;
        if (needed < p.blocks && !batch) p.blocks = (int)(needed > 0 ? needed : 1);
    }
    a.spill_entries = sc.view.stack_need > kLdsStackEntries ? sc.view.stack_need - kLdsStackEntries : 0;
    a.spill_stride = (uint32_t)((size_t)p.blocks * kThreadsPerBlock);                  // lanes
    a.min_walk_iters = desc->tune[0] > 0 ? desc->tune[0] : 64;      // (192 when the rays walk the certified second tree: set below, once a.accel is known)
    a.advance_budget = desc->tune[1] > 0 ? desc->tune[1] : 12;
    a.leaf_ratio4 = desc->tune[2] > 0 ? desc->tune[2] : 10;            // (16 until the node loop looked at its votes every other iteration: profiles/r03/ab_loop_knobs_after_unroll.jsonl)
    a.deal_leaves = (xp & 128u) ? 0 : 1;
    // The certified second tree (pack_scene): used when it is resident, the host has not asked for the plain reference walk, and every camera of the launch is within
    // 30 scene extents of the scene's centre (the widening of the second tree's boxes covers the rounding of (box - origin) up to there; bounce and shadow rays start
    // on the geometry).  Otherwise every ray walks the reference tree, as without the option.
    a.accel = 0;
    if (sc.has_second_tree && !(flags & DSRT_TUNE_REFERENCE_WALK)) {
        auto near_enough = [&](const DsrtF3& o) {
            const double dx = (double)o.x - sc.scene_centre[0], dy = (double)o.y - sc.scene_centre[1], dz = (double)o.z - sc.scene_centre[2];
            return std::sqrt(dx * dx + dy * dy + dz * dz) <= 30.0 * (double)sc.scene_extent;
        };
        bool ok = true;
        if (batch) { for (int i = 0; i < batch->frames && ok; ++i) ok = near_enough(batch->cameras[i].origin); }
        else ok = near_enough(fs.camera.origin);
        a.accel = ok ? 1 : 0;
    }
    a.audit = a.accel && desc->collect_counters == 3 ? 1 : 0;
    // Walks of the second tree are a third shorter, so an advance pass is dearer against a node iteration than on the reference tree: the traverse phase stays three times
    // longer before it yields (interleaved medians, near frame: 760 -> 741 ms in rng_mode 0, 734 -> 701 in rng_mode 1; the reference walk gains nothing from it).
    if (a.accel && desc->tune[0] <= 0) a.min_walk_iters = 192;
    // ... and its leaves come sooner: the node loop yields to the leaf pass at 0.6 parked lane-slots per descending lane instead of 1.0 (rng_mode 0: near frame -0.5 ... -1.1 %,
    // frame 85 -5 %, frame 92 -2 %, one of 8 shares -1.6 %, far frames unchanged; rng_mode 1 loses 1 % and keeps 1.0: profiles/r04/ab_leaf_ratio_*.jsonl).
    if (a.accel && desc->rng_mode == 0 && desc->tune[2] <= 0) a.leaf_ratio4 = 6;
    a.helpers = (flags & DSRT_TUNE_NO_HELPERS) ? 0 : 1;
    a.steal = ((flags & DSRT_TUNE_NO_STEALING) ? 0 : 1) | (((xp & (1u << 27)) && desc->collect_counters) ? 8 : 0);      // (8: timing image, counting build)
    // rng_mode 0: waves that hold a pixel of a heavy tile get issue priority over waves that only hold background pixels (render_body).
    // Interleaved medians, 1080p x 1000: near frame 1117 -> 1108 ms, frame 95 801 -> 785 ms.  Finer grades (the top quarter and sixteenth of
    // the order above the rest) were tried in round 2 and moved nothing consistently (profiles/r02/ab_issue_priority.jsonl); they are gone.
    a.hot = (flags & DSRT_TUNE_NO_PRIORITY) ? 0 : 1;

    // Pre-pass for this camera: costliest-first tile order (scheduling only) and removal of tiles that are provably empty (exact:
    // see dsrt_tile_cost_kernel).  DSRT_TUNE_NATURAL_ORDER switches both off, DSRT_TUNE_NO_CULLING keeps the order but culls nothing; counting builds never
    // cull, so that their counters cover every sample.  The words 32 and 48 entries past the cost array receive the number of
    // tiles that see geometry and the number of tiles in the order.
    p.pre_stride = (size_t)t.mine + 64;
    if (p.pre_stride * (size_t)p.frames >= ((size_t)1 << 32)) { set_error("dsrt_render_batch: too many tiles in one batch (split the sequence)"); return DSRT_ERR_INVALID; }
    p.pre = batch ? PrePass::Batch : ((flags & 3u) != DSRT_TUNE_NATURAL_ORDER && t.mine > 0 ? PrePass::Ordered : PrePass::Natural);
    p.cull = batch ? (flags & 3u) == 0u : (flags & 3u) != DSRT_TUNE_NO_CULLING && desc->collect_counters == 0;
    // The probe (probe_tiles) is worth its 0.5 % only when a pixel is a long chain; DSRT_TUNE_NO_PROBE switches it off.
    // Only with the reference's stream: in rng_mode 1 a pixel is cut into slices and lanes share samples, so there is no long chain to start
    // early, and the coverage order alone is better (interleaved medians, near frame: 1046 -> 1037 ms, one of 8 shares 176 -> 167 ms).
    p.probe = p.pre != PrePass::Natural && !(flags & DSRT_TUNE_NO_PROBE) && desc->rng_mode == 0 && f.spp >= 64 * kProbeSpp;
    p.probe_spp = (!batch && (xp & 64u)) ? 2 * kProbeSpp : kProbeSpp;                  // experiment (a batch's probes ignore it)

    const bool count = desc->collect_counters != 0;
    RenderVariant& v = p.variant;
    v = RenderVariant{};
    v.rng_mode = desc->rng_mode;
    v.count = count; v.checked = count || desc->checked != 0; v.anyhit = desc->collect_counters != 2;
    v.lean = lean; v.sets = acc != nullptr; v.moments = acc && acc->sum_sq; v.listed = acc && acc->mask;
    return DSRT_OK;
}

// Each buffer by its own size: a failed allocation leaves no stale sibling.
static int grow_render_buffers(DsrtContext* ctx, RenderPlan& p) {
    RenderArgs& a = p.a;
    int rc;
    if (p.own_sums) {
        if ((rc = ctx->accum_fixed.grow(p.out_pixels * 3))) return rc;
        a.accum_fixed = ctx->accum_fixed.p;
    }
    if (a.spill_entries > 0 && (rc = ctx->spill.grow((size_t)a.spill_stride * (size_t)a.spill_entries))) return rc;
    a.spill = ctx->spill.p;
    if ((rc = ctx->tile_cost.grow(p.pre_stride * (size_t)p.frames)) || (rc = ctx->tile_order.grow(p.pre_stride * (size_t)p.frames)) ||
        (rc = ctx->tile_work.grow(p.pre_stride)) || (rc = ctx->tile_tmp.grow(p.pre_stride))) return rc;
    if (p.pre == PrePass::Batch && (rc = ctx->batch_table.grow(2 * (size_t)p.frames))) return rc;
    if (p.probe && (rc = ctx->probe_queue.grow(1024))) return rc;
    if (p.variant.listed) {
        const size_t tile_pixels = (size_t)p.t.mine * (size_t)(p.t.tile * p.t.tile);     // the two lists, and a word per 8x8 block behind them (launch_pixel_list)
        if ((rc = ctx->pixel_list.grow(tile_pixels + tile_pixels / 64))) return rc;
        a.list = ctx->pixel_list.p;
    }
    p.sched = ctx->tile_cost.p + p.t.mine + 32;
    a.sched = p.sched;
    if (p.variant.listed) a.list_len = p.sched + kListLenSched;
    return DSRT_OK;
}

// Probe: the render kernel itself at a few samples per pixel (reference stream, nothing stored) measures what every tile of the frame `pa` describes
// costs; the heavy tiles of its order (`at` entries into the context's order and sched arrays) are then re-sorted by that.
// Its work items are tiny, so the probe has 64 queue words of its own (path_machine.h, ST_FETCH): on the frame's single queue word
// the same launch took 27 ms.  It leaves the frame's queue words used: the caller zeroes `ctrl` behind its last probe, and, where probes follow each
// other, before each (zero_ctrl_first).
static int probe_tiles(DsrtContext* ctx, const RenderPlan& p, RenderArgs pa, size_t at, bool zero_ctrl_first, hipStream_t stream) {
    pa.frame.spp = p.probe_spp;
    pa.out_f32 = nullptr; pa.accum_fixed = nullptr; pa.counters = nullptr;
    pa.sched = p.sched + at;
    pa.frame.tile_order = ctx->tile_order.p + at;
    pa.tile_work = ctx->tile_work.p;
    pa.probe_queue = ctx->probe_queue.p;
    HIP_TRY(hipMemsetAsync(ctx->probe_queue.p, 0, 1024 * sizeof(uint32_t), stream));
    HIP_TRY(hipMemsetAsync(ctx->tile_work.p, 0, (size_t)p.t.mine * sizeof(uint32_t), stream));
    if (zero_ctrl_first) HIP_TRY(hipMemsetAsync(ctx->ctrl.p, 0, kCtrlWords * sizeof(uint32_t), stream));
    HIP_TRY(p.rl->launch_probe(pa, p.blocks, p.variant.lean, stream));
    HIP_TRY(launch_tile_reorder(ctx->tile_work.p, ctx->tile_order.p + at, ctx->tile_tmp.p, p.sched + at, stream));
    return DSRT_OK;
}

// Batch: every frame's pre-pass (exact culling + coverage order), its results left pre_stride apart; then one small kernel turns the counts into the
// table the render kernel looks work items up in.  Slices stay at the host's 8 (resident_lanes = 0: the pool is never short of heavy pixels).
static int prepass_batch(DsrtContext* ctx, RenderPlan& p, const BatchInput& batch, hipStream_t stream) {
    RenderArgs& a = p.a;
    const size_t frames = (size_t)p.frames;
    HIP_TRY(hipMemsetAsync(a.out_rgb8, 0, p.out_pixels * 3, stream));                          // culled pixels are never written
    if (a.out_f32) HIP_TRY(hipMemsetAsync(a.out_f32, 0, p.out_pixels * 3 * sizeof(float), stream));
    ctx->batch_host.assign(2 * frames, BatchFrame{});
    for (size_t i = 0; i < frames; ++i) {
        BatchFrame& e = ctx->batch_host[i];
        pack_camera(batch.cameras[i], e.cam);
        e.sun_dir[0] = batch.sun_dirs[i].x; e.sun_dir[1] = batch.sun_dirs[i].y; e.sun_dir[2] = batch.sun_dirs[i].z;
        e.order_base = (uint32_t)(p.pre_stride * i);
        e.image_slot = (uint32_t)i;
        ctx->batch_host[frames + i] = e;                                                  // the frame's second entry (device_layout.h, BatchFrame)
    }
    HIP_TRY(hipMemcpyAsync(ctx->batch_table.p, ctx->batch_host.data(), 2 * frames * sizeof(BatchFrame), hipMemcpyHostToDevice, stream));
    HIP_TRY(launch_tile_order(a.scene, a.frame, ctx->tile_cost.p, ctx->tile_order.p, p.sched, (uint32_t)p.chunks, 0u, p.cull, stream,
                              ctx->batch_table.p, (uint32_t)frames, (uint32_t)p.pre_stride));
    // rng_mode 0 at enough samples for a pixel to be a long chain: every frame's heavy tiles re-sorted by measured cost, as for a single
    // frame -- one probe per frame, 6 ms each at 1080p, against a frame of a second
    if (p.probe) {
        for (size_t i = 0; i < frames; ++i) {
            RenderArgs pa = a;
            std::memcpy(pa.frame.cam, ctx->batch_host[i].cam, sizeof pa.frame.cam);
            std::memcpy(pa.frame.sun_dir, ctx->batch_host[i].sun_dir, 3 * sizeof(float));
            if (int rc = probe_tiles(ctx, p, pa, p.pre_stride * i, true, stream)) return rc;
        }
        HIP_TRY(hipMemsetAsync(ctx->ctrl.p, 0, kCtrlWords * sizeof(uint32_t), stream));
    }
    HIP_TRY(launch_batch_table(ctx->batch_table.p, p.sched, (uint32_t)p.pre_stride, (uint32_t)frames, (uint32_t)(p.t.tile * p.t.tile), p.variant.rng_mode, a.frame.spp,
                               a.frame.light_chunk_len, ctx->ctrl.p + 2, stream));
    a.batch = ctx->batch_table.p; a.batch_order = ctx->tile_order.p; a.batch_frames = 2u * (uint32_t)frames;
    a.batch_frame_pixels = (uint32_t)(p.out_pixels / frames);        // whole images, or the padded compact shard buffers, one after another
    return DSRT_OK;
}

// One frame, costliest tiles first.
static int prepass_ordered(DsrtContext* ctx, RenderPlan& p, hipStream_t stream) {
    RenderArgs& a = p.a;
    if (p.cull && a.out_rgb8) {                                 // culled pixels are never written: they are the zeros put here (an accumulate launch adds nothing for them)
        HIP_TRY(hipMemsetAsync(a.out_rgb8, 0, p.out_pixels * 3, stream));
        if (a.out_f32) HIP_TRY(hipMemsetAsync(a.out_f32, 0, p.out_pixels * 3 * sizeof(float), stream));
    }
    HIP_TRY(launch_tile_order(a.scene, a.frame, ctx->tile_cost.p, ctx->tile_order.p, p.sched, (uint32_t)p.chunks,
                              (uint32_t)p.blocks * (uint32_t)kThreadsPerBlock, p.cull, stream));
    a.frame.tile_order = ctx->tile_order.p;
    if (p.probe) {
        if (int rc = probe_tiles(ctx, p, a, 0, false, stream)) return rc;
        HIP_TRY(hipMemsetAsync(ctx->ctrl.p, 0, kCtrlWords * sizeof(uint32_t), stream));
    }
    return DSRT_OK;
}

// One frame, every tile in the heavy queue, natural order.
static int prepass_natural(const RenderPlan& p, hipStream_t stream) {
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)p.sched, p.t.mine, 2, stream));
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)(p.sched + 2), 64, 1, stream));
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)(p.sched + 3), p.chunks, 1, stream));
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)(p.sched + 4), p.chunk_len, 1, stream));
    return DSRT_OK;
}

static int launch_and_resolve(const RenderPlan& p, hipStream_t stream) {
    const RenderArgs& a = p.a;
    if (p.pre == PrePass::Batch) HIP_TRY(p.rl->launch_render_batch(a, p.variant.rng_mode, p.blocks, p.variant.lean, stream));
    else HIP_TRY(p.rl->launch_render(a, p.variant, p.blocks, stream));
    if (p.own_sums) HIP_TRY(p.rl->launch_resolve(a.accum_fixed, a.frame.spp, a.frame.inv_gamma, p.out_pixels, a.out_rgb8, a.out_f32, nullptr, nullptr, stream));
    return DSRT_OK;
}

// The counters of a finished launch (launch_finish has waited for it), as DsrtStats.
static int read_render_stats(DsrtContext* ctx, const RenderPlan& p, DsrtStats* stats) {
    uint32_t ctrl[kCtrlWords];
    HIP_TRY(hipMemcpy(ctrl, ctx->ctrl.p, sizeof ctrl, hipMemcpyDeviceToHost));
    stats->device_flags = ctrl[1];
    stats->waves_launched = p.blocks * kWavesPerBlock;
    stats->lds_stack_entries = kLdsStackEntries;
    uint64_t cnt[kNumCounters];
    std::memcpy(cnt, &ctrl[4], sizeof cnt);
    stats->samples = cnt[C_SAMPLES]; stats->rays = cnt[C_RAYS]; stats->primary_hits = cnt[C_PRIMARY_HITS];
    stats->box_fetches = cnt[C_BOX_FETCHES]; stats->nodes_entered = cnt[C_NODES_ENTERED]; stats->internal_entered = cnt[C_INTERNAL_ENTERED];
    stats->tri_tests = cnt[C_TRI_TESTS]; stats->hit_updates = cnt[C_HIT_UPDATES]; stats->sphere_tests = cnt[C_SPHERE_TESTS];
    stats->shaded_hits = cnt[C_SHADED_HITS]; stats->tex_fetches = cnt[C_TEX_FETCHES]; stats->stack_spills = cnt[C_STACK_SPILLS];
    stats->max_stack = cnt[C_MAX_STACK];
    stats->node_slots = cnt[C_NODE_SLOTS]; stats->tri_slots = cnt[C_TRI_SLOTS]; stats->adv_slots = cnt[C_ADV_SLOTS]; stats->adv_active = cnt[C_ADV_ACTIVE];
    stats->idle_at_leaf = cnt[C_IDLE_AT_LEAF]; stats->idle_waiting = cnt[C_IDLE_WAITING]; stats->idle_done = cnt[C_IDLE_DONE];
    stats->wave_ticks = cnt[C_WAVE_TICKS];
    stats->certificate_fallbacks = cnt[C_CERT_FALLBACKS];
    stats->certificate_audited = cnt[C_AUDITED]; stats->certificate_audit_mismatches = cnt[C_AUDIT_MISMATCHES];
    stats->certified_tree_used = p.a.accel;
    {   // time marks relative to the first wave's start, in ms (0 when the mark was never passed)
        const double t0 = (double)~cnt[C_T_FIRST];
        stats->heavy_queue_empty_ms = cnt[C_T_HEAVY_EMPTY] ? (float)(((double)~cnt[C_T_HEAVY_EMPTY] - t0) * 1e-5) : 0.0f;
        stats->light_queue_empty_ms = cnt[C_T_LIGHT_EMPTY] ? (float)(((double)~cnt[C_T_LIGHT_EMPTY] - t0) * 1e-5) : 0.0f;
        stats->last_wave_exit_ms = cnt[C_T_LAST] ? (float)(((double)cnt[C_T_LAST] - t0) * 1e-5) : 0.0f;
    }
    stats->visits_depth_lt6 = cnt[C_VISITS_LT6]; stats->visits_depth_lt9 = cnt[C_VISITS_LT9]; stats->visits_depth_lt12 = cnt[C_VISITS_LT12];
    uint32_t live = 0;
    HIP_TRY(hipMemcpy(&live, p.sched + 1, sizeof live, hipMemcpyDeviceToHost));
    stats->tiles_total = (uint64_t)p.t.mine; stats->tiles_culled = (uint64_t)p.t.mine - live;
    return DSRT_OK;
}

static int render_impl(DsrtContext* ctx, const DsrtRenderDesc* desc, uint8_t* d_rgb8, float* d_f32, void* stream_v, DsrtStats* stats, const BatchInput* batch,
                              const AccumInput* acc = nullptr) {
    RenderPlan p;
    int rc = plan_render(ctx, desc, d_rgb8, d_f32, batch, acc, p);          // every refusal: nothing has been enqueued
    if (rc) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t stream = (hipStream_t)stream_v;
    if ((rc = grow_render_buffers(ctx, p))) return rc;
    // a context's working buffers serve one render at a time; its own sums (24 bytes per pixel) and its queue, flag and counter words start at zero
    if ((rc = launch_begin(ctx, stream, {{p.own_sums ? p.a.accum_fixed : nullptr, p.out_pixels * 3 * sizeof(unsigned long long)}, {ctx->ctrl.p, kCtrlWords * sizeof(uint32_t)}}))) return rc;
    switch (p.pre) {
        case PrePass::Batch: rc = prepass_batch(ctx, p, *batch, stream); break;
        case PrePass::Ordered: rc = prepass_ordered(ctx, p, stream); break;
        case PrePass::Natural: rc = prepass_natural(p, stream); break;
    }
    // a masked launch: the lists of active pixels, from the mask and the order the pre-pass has just left (and the sample counts of those pixels)
    if (!rc && p.variant.listed)
        HIP_TRY(launch_pixel_list(p.a.frame, p.a.frame.tile_order, p.sched, acc->mask, ctx->pixel_list.p, p.sched + kListLenSched, acc->n, (uint32_t)acc->count, stream));
    if (rc || (rc = launch_clock(ctx, stream, stats)) || (rc = launch_and_resolve(p, stream)) || (rc = launch_finish(ctx, stream, stats)) || !stats) return rc;
    if ((rc = read_render_stats(ctx, p, stats))) return rc;
    return flags_result("render", stats->device_flags);
}

int dsrt_ctx_scene_bounds(const DsrtContext* ctx, float lo[3], float hi[3]) {
    if (!ctx || !lo || !hi) { set_error("dsrt_ctx_scene_bounds: null argument"); return DSRT_ERR_INVALID; }
    const PackedScene* sc = resident_scene(ctx, "dsrt_ctx_scene_bounds");
    if (!sc) return DSRT_ERR_NO_SCENE;
    for (int a = 0; a < 3; ++a) { lo[a] = sc->view.root_lo[a]; hi[a] = sc->view.root_hi[a]; }
    return DSRT_OK;
}

int dsrt_render(DsrtContext* ctx, const DsrtRenderDesc* desc, uint8_t* d_rgb8, float* d_f32, void* stream, DsrtStats* stats) {
    return render_impl(ctx, desc, d_rgb8, d_f32, stream, stats, nullptr);
}

int dsrt_render_batch(DsrtContext* ctx, const DsrtRenderDesc* desc, int frames, const GPUCamera* cameras, const float* sun_dirs_xyz, uint8_t* d_rgb8, float* d_f32,
                      void* stream, DsrtStats* stats) {
    return dsrt::guarded("dsrt_render_batch", [&]() -> int {
        if (frames < 1 || !cameras || !sun_dirs_xyz) { set_error("dsrt_render_batch: null argument"); return DSRT_ERR_INVALID; }
        std::vector<DsrtF3> suns((size_t)frames);
        for (int i = 0; i < frames; ++i) suns[(size_t)i] = DsrtF3{sun_dirs_xyz[3 * i], sun_dirs_xyz[3 * i + 1], sun_dirs_xyz[3 * i + 2]};
        const BatchInput b{frames, cameras, suns.data()};
        return render_impl(ctx, desc, d_rgb8, d_f32, stream, stats, &b);
    });
}

int dsrt_deinterleave_batch(DsrtContext* ctx, const DsrtRenderDesc* desc, int frames, const uint8_t* d_gathered, uint8_t* d_rgb8_images, void* stream) {
    Tiling t;
    if (!ctx || !desc || frames < 1 || !d_gathered || !d_rgb8_images || !make_tiling(*desc, t)) { set_error("dsrt_deinterleave_batch: bad argument"); return DSRT_ERR_INVALID; }
    HIP_TRY(hipSetDevice(ctx->device));
    const int count = desc->shard_count > 1 ? desc->shard_count : 1;
    const size_t part = (size_t)t.padded * t.tile * t.tile * 3, image = (size_t)desc->width * desc->height * 3;
    // the gather of sharded batch launches: rank r's buffer holds its part of frame 0, of frame 1, ...; rank r + 1's follows `frames` parts on
    for (int f = 0; f < frames; ++f)
        HIP_TRY(launch_deinterleave(d_gathered + (size_t)f * part, d_rgb8_images + (size_t)f * image, desc->width, desc->height, t.tile, t.tiles_x, count,
                                    part * (size_t)frames, (hipStream_t)stream));
    return DSRT_OK;
}

int dsrt_deinterleave_tiles(DsrtContext* ctx, const DsrtRenderDesc* desc, const uint8_t* d_gathered, uint8_t* d_rgb8_image, void* stream) {
    Tiling t;
    if (!ctx || !desc || !d_gathered || !d_rgb8_image || !make_tiling(*desc, t)) { set_error("dsrt_deinterleave_tiles: bad argument"); return DSRT_ERR_INVALID; }
    HIP_TRY(hipSetDevice(ctx->device));
    const int count = desc->shard_count > 1 ? desc->shard_count : 1;
    HIP_TRY(launch_deinterleave(d_gathered, d_rgb8_image, desc->width, desc->height, t.tile, t.tiles_x, count, (size_t)t.padded * t.tile * t.tile * 3,
                                (hipStream_t)stream));
    return DSRT_OK;
}

int dsrt_render_batch_to_host(DsrtContext* ctx, const DsrtRenderDesc* desc, int frames, const GPUCamera* cameras, const float* sun_dirs_xyz, uint8_t* h_rgb8,
                              DsrtStats* stats) {
    return dsrt::guarded("dsrt_render_batch_to_host", [&]() -> int {
    if (!ctx || !desc || !h_rgb8 || frames < 1) { set_error("dsrt_render_batch_to_host: null argument"); return DSRT_ERR_INVALID; }
    HIP_TRY(hipSetDevice(ctx->device));
    const Staged s[1] = {{h_rgb8, (size_t)desc->width * desc->height * 3 * (size_t)frames, Dir::Out}};
    DsrtStats local;
    return staged_call(s, [&](void* const* d) { return dsrt_render_batch(ctx, desc, frames, cameras, sun_dirs_xyz, (uint8_t*)d[0], nullptr, nullptr, stats ? stats : &local); });
    });
}

int dsrt_render_to_host(DsrtContext* ctx, const DsrtRenderDesc* desc, uint8_t* h_rgb8, float* h_f32, DsrtStats* stats) {
    return dsrt::guarded("dsrt_render_to_host", [&]() -> int {
    if (!ctx || !desc || !h_rgb8) { set_error("dsrt_render_to_host: null argument"); return DSRT_ERR_INVALID; }
    if (desc->shard_count > 1) { set_error("dsrt_render_to_host renders whole images only"); return DSRT_ERR_INVALID; }
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t px = (size_t)desc->width * desc->height;
    const Staged s[2] = {{h_rgb8, px * 3, Dir::Out}, {h_f32, px * 3 * sizeof(float), Dir::Out}};
    DsrtStats local;
    return staged_call(s, [&](void* const* d) { return dsrt_render(ctx, desc, (uint8_t*)d[0], (float*)d[1], nullptr, stats ? stats : &local); });
    });
}

// ---- Sample sets (include/dsrt.h, dsrt_render_accumulate): rng_mode 1 sums of any set of a pixel's samples, added into caller-owned buffers ----
namespace {
int accum_fail(const char* fn, const char* why) { set_error(std::string(fn) + ": " + why); return DSRT_ERR_INVALID; }
// (`static` below: inside extern "C" a function of an unnamed namespace keeps its plain name, and without it the library would export that name)

// What every entry point over a frame's sums refuses of `desc`, checked like everything below before any HIP call and before anything is written.  Where the
// entry points differ, a parameter says so: a launch that renders (`renders`) words the rng_mode refusal for its caller and leaves math_mode and the size to
// plan_render; the denoiser numbers pixels with 31 bits (`limit_2_31`).  (samples_done: check_sums, check_denoise; collect_counters: check_masked_desc.)
static int check_frame_desc(const char* fn, const DsrtRenderDesc* desc, bool renders, bool limit_2_31) {
    if (desc->rng_mode != 1) return accum_fail(fn, renders ? "sample sets need rng_mode 1 (rng_mode 0 draws a pixel's samples from one serial stream)" : "accumulated sums are rng_mode 1's");
    if (!renders && desc->math_mode != 0 && desc->math_mode != 1) return accum_fail(fn, "math_mode must be 0 or 1");
    if (desc->shard_count > 1) return accum_fail(fn, "sample sets of tile shards (shard_count > 1) are not supported");
    if (!renders && (desc->width < 2 || desc->height < 2)) return accum_fail(fn, "width and height must be >= 2");
    if (limit_2_31 && (unsigned long long)desc->width * (unsigned long long)desc->height >= (1ull << 31)) return accum_fail(fn, "image too large (2^31 pixels)");
    return DSRT_OK;
}

// Everything dsrt_render_accumulate refuses: of the context, the frame and the set (ctx and desc are given) ...
int check_sample_set(const char* fn, const DsrtContext* ctx, const DsrtRenderDesc* desc, int first, int count, int stride) {
    if (!resident_scene(ctx, fn)) return DSRT_ERR_NO_SCENE;
    if (int rc = check_frame_desc(fn, desc, true, false)) return rc;
    if (first < 0) return accum_fail(fn, "first < 0");
    if (count < 1) return accum_fail(fn, "count < 1");
    if (stride < 1) return accum_fail(fn, "stride < 1");
    const long long spp = desc->spp < 1 ? 1 : desc->spp;
    if ((long long)first + (long long)(count - 1) * (long long)stride >= spp) return accum_fail(fn, "the set reaches past the frame's planned samples (first + (count - 1) * stride >= spp)");
    return DSRT_OK;
}

int check_masked_desc(const char* fn, const DsrtRenderDesc* desc) {
    if (desc->collect_counters != 0) return accum_fail(fn, "masked launches use the production and checked kernels only (collect_counters must be 0)");
    return DSRT_OK;
}

// ... and of the sums; a masked launch (`masked`: dsrt_render_accumulate_masked) needs its mask too.
int check_accumulate(const char* fn, const DsrtContext* ctx, const DsrtRenderDesc* desc, int first, int count, int stride, const DsrtAccum* acc, bool masked, const uint8_t* mask) {
    if (!ctx || !desc || !acc) return accum_fail(fn, "null argument");
    if (!acc->sum) return accum_fail(fn, "DsrtAccum.sum is NULL (it is required; sum_sq is the optional one)");
    if (int rc = check_sample_set(fn, ctx, desc, first, count, stride)) return rc;
    if (!masked) return DSRT_OK;
    if (!mask) return accum_fail(fn, "the mask is NULL (dsrt_render_accumulate renders every pixel)");
    return check_masked_desc(fn, desc);
}

// dsrt_render_accumulate and (`masked`) dsrt_render_accumulate_masked: mask (null = every pixel) and n as AccumInput has them ...
static int accumulate_impl(const char* fn, DsrtContext* ctx, const DsrtRenderDesc* desc, int first, int count, int stride, const DsrtAccum* acc, bool masked, const uint8_t* d_mask,
                           uint32_t* d_n, void* stream, DsrtStats* stats) {
    if (int rc = check_accumulate(fn, ctx, desc, first, count, stride, acc, masked, d_mask)) return rc;
    const AccumInput in{first, count, stride, (unsigned long long*)acc->sum, (unsigned long long*)acc->sum_sq, d_mask, d_n};
    return render_impl(ctx, desc, nullptr, nullptr, stream, stats, nullptr, &in);
}

// ... and their _to_host forms: sums and counts in and out.
struct AccumMirrors { DsrtAccum acc; const uint8_t* mask; uint32_t* n; };        // the staged list below, by name
static int accumulate_to_host(const char* fn, DsrtContext* ctx, const DsrtRenderDesc* desc, int first, int count, int stride, const DsrtAccum* h_acc, bool masked, const uint8_t* h_mask,
                              uint32_t* h_n, DsrtStats* stats) {
    if (int rc = check_accumulate(fn, ctx, desc, first, count, stride, h_acc, masked, h_mask)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t px = (size_t)desc->width * desc->height;
    const Staged s[4] = {{h_acc->sum, px * 3 * sizeof(uint64_t), Dir::InOut}, {h_acc->sum_sq, px * 3 * sizeof(uint64_t), Dir::InOut}, {h_mask, px, Dir::In},
                         {h_n, px * sizeof(uint32_t), Dir::InOut}};
    DsrtStats local;
    return staged_call(s, [&](void* const* d) {
        const AccumMirrors m = pointers_as<AccumMirrors>(d);
        return accumulate_impl(fn, ctx, desc, first, count, stride, &m.acc, masked, m.mask, m.n, nullptr, stats ? stats : &local);
    });
}

// What the two resolves, dsrt_select_unconverged and the adaptive driver refuse.  The checks ask whether a buffer is given, never what it holds: have_args (acc, and the
// counts where they are needed), have_sum, have_sq say so (the adaptive _to_host driver checks before it has allocated any).  `samples_done`: null where per-pixel counts
// stand in for it; `outputs`: the resolve's three, null for the convergence test, whose output is the mask.
static int check_sums(const char* fn, const DsrtContext* ctx, const DsrtRenderDesc* desc, bool have_args, bool have_sum, bool have_sq, const int* samples_done, bool need_sq,
                      const void* const* outputs) {
    if (!ctx || !desc || !have_args) return accum_fail(fn, "null argument");
    if (!have_sum) return accum_fail(fn, "DsrtAccum.sum is NULL");
    if (int rc = check_frame_desc(fn, desc, false, false)) return rc;
    if (samples_done && *samples_done < 1) return accum_fail(fn, "samples_done < 1");
    if (need_sq && !have_sq) return accum_fail(fn, "the variance needs DsrtAccum.sum_sq");
    if (outputs && !outputs[0] && !outputs[1] && !outputs[2]) return accum_fail(fn, "no output");
    if (samples_done && need_sq && *samples_done < 2) return accum_fail(fn, "the variance needs samples_done >= 2");
    return DSRT_OK;
}

// dsrt_resolve_accumulated and dsrt_resolve_accumulated_counts: every pixel's count is samples_done, or (`per_pixel`) its own entry of d_n.
static int resolve_sums(const char* fn, DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtAccum* acc, bool per_pixel, int samples_done, const uint32_t* d_n, uint8_t* d_rgb8,
                        float* d_f32, float* d_var_of_mean, hipStream_t stream) {
    const void* outputs[3] = {d_rgb8, d_f32, d_var_of_mean};
    int rc = check_sums(fn, ctx, desc, acc && (d_n || !per_pixel), acc && acc->sum, acc && acc->sum_sq, per_pixel ? nullptr : &samples_done, d_var_of_mean != nullptr, outputs);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    if ((rc = launch_begin(ctx, stream, {}))) return rc;                             // the context's last launch (an accumulate into these sums, maybe) comes first
    const RenderLaunchers& rl = render_launchers(desc->math_mode == 1);
    const size_t px = (size_t)desc->width * desc->height;
    const unsigned long long* sum = (const unsigned long long*)acc->sum;
    const unsigned long long* sq = d_var_of_mean ? (const unsigned long long*)acc->sum_sq : nullptr;       // (the second moment serves the variance only)
    HIP_TRY(per_pixel ? rl.launch_resolve_counts(sum, d_n, inv_gamma_of(*desc), px, d_rgb8, d_f32, sq, d_var_of_mean, stream)
                      : rl.launch_resolve(sum, samples_done, inv_gamma_of(*desc), px, d_rgb8, d_f32, sq, d_var_of_mean, stream));
    return DSRT_OK;
}

// The table's entries [from, to) against those before them and among themselves: alignment; then each of their outputs against every input up to `to` (over_input) and
// against every other output not checked against it yet (over_output); then the outputs before `from` against their inputs (old_over_input; nothing to do for from = 0).
static int check_frame_table(const char* fn, const Staged (&s)[kFrameBufferCount], size_t from, size_t to, const char* over_input, const char* over_output, const char* old_over_input) {
    for (size_t k = from; k < to; ++k)
        if ((uintptr_t)s[k].host & (kFrameBuffers[k].align - 1))
            return accum_fail(fn, kFrameBuffers[k].align == 8 ? "a sum pointer is not 8-byte aligned" : kFrameBuffers[k].align == 16 ? "a history buffer is not 16-byte aligned" : "pointer not 4-byte aligned");
    for (size_t a = from; a < to; ++a) {
        if (s[a].dir != Dir::Out) continue;
        for (size_t i = 0; i < to; ++i) if (s[i].dir == Dir::In && ranges_overlap(s[a], s[i])) return accum_fail(fn, over_input);
        for (size_t b = 0; b < to; ++b) if (s[b].dir == Dir::Out && (b < from || b > a) && ranges_overlap(s[a], s[b])) return accum_fail(fn, over_output);
    }
    for (size_t a = 0; a < from; ++a)
        for (size_t i = from; i < to; ++i) if (s[a].dir == Dir::Out && s[i].dir == Dir::In && ranges_overlap(s[a], s[i])) return accum_fail(fn, old_over_input);
    return DSRT_OK;
}

// A frame's sums, counts and guides on the device for the length of a _to_host call, sums and counts zeroed, with the views of them the entry points take.
struct FrameScratch {
    DevBuf<unsigned long long> sum, sq;
    DevBuf<uint32_t> n;
    DevBuf<float> normal, position, albedo, range;
    DsrtAccum acc{};
    DsrtDenoiseGuides guides{};
    DsrtGBuffer gb{};                                                  // the guides' four channels and no other
    int init(size_t px, bool counts, bool with_guides) {
        int rc;
        if ((rc = sum.alloc(px * 3)) || (rc = sq.alloc(px * 3)) || (counts && (rc = n.alloc(px)))) return rc;
        if (with_guides && ((rc = normal.alloc(px * 3)) || (rc = position.alloc(px * 3)) || (rc = albedo.alloc(px * 3)) || (rc = range.alloc(px)))) return rc;
        HIP_TRY(hipMemset(sum.p, 0, px * 3 * sizeof(unsigned long long)));
        HIP_TRY(hipMemset(sq.p, 0, px * 3 * sizeof(unsigned long long)));
        if (counts) HIP_TRY(hipMemset(n.p, 0, px * sizeof(uint32_t)));
        acc = DsrtAccum{(uint64_t*)sum.p, (uint64_t*)sq.p};
        guides = DsrtDenoiseGuides{normal.p, position.p, albedo.p, range.p};
        gb.normal = normal.p; gb.position = position.p; gb.albedo = albedo.p; gb.range = range.p;
        return DSRT_OK;
    }
};
}  // namespace

int dsrt_render_accumulate(DsrtContext* ctx, const DsrtRenderDesc* desc, int first, int count, int stride, const DsrtAccum* acc, void* stream, DsrtStats* stats) {
    return dsrt::guarded("dsrt_render_accumulate", [&]() -> int {
    return accumulate_impl("dsrt_render_accumulate", ctx, desc, first, count, stride, acc, false, nullptr, nullptr, stream, stats);
    });
}

int dsrt_render_accumulate_to_host(DsrtContext* ctx, const DsrtRenderDesc* desc, int first, int count, int stride, const DsrtAccum* h_acc, DsrtStats* stats) {
    return dsrt::guarded("dsrt_render_accumulate_to_host", [&]() -> int {
    return accumulate_to_host("dsrt_render_accumulate_to_host", ctx, desc, first, count, stride, h_acc, false, nullptr, nullptr, stats);
    });
}

int dsrt_resolve_accumulated(DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtAccum* acc, int samples_done, uint8_t* d_rgb8, float* d_f32,
                             float* d_var_of_mean, void* stream_v) {
    return dsrt::guarded("dsrt_resolve_accumulated", [&]() -> int {
    return resolve_sums("dsrt_resolve_accumulated", ctx, desc, acc, false, samples_done, nullptr, d_rgb8, d_f32, d_var_of_mean, (hipStream_t)stream_v);
    });
}

int dsrt_resolve_accumulated_to_host(DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtAccum* h_acc, int samples_done, uint8_t* h_rgb8, float* h_f32,
                                     float* h_var_of_mean) {
    return dsrt::guarded("dsrt_resolve_accumulated_to_host", [&]() -> int {
    const void* outputs[3] = {h_rgb8, h_f32, h_var_of_mean};
    if (int rc = check_sums("dsrt_resolve_accumulated_to_host", ctx, desc, h_acc != nullptr, h_acc && h_acc->sum, h_acc && h_acc->sum_sq, &samples_done, h_var_of_mean != nullptr, outputs))
        return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    FrameBuffers h{};
    h.sum = h_acc->sum; h.sum_sq = h_var_of_mean ? h_acc->sum_sq : nullptr;          // (the second moment serves the variance only)
    h.rgb8 = h_rgb8; h.f32 = h_f32; h.var = h_var_of_mean;
    return staged_frame_call(h, (size_t)desc->width * desc->height, false, [&](const FrameBuffers& m) {
        const DsrtAccum acc = accum_of(m);
        return dsrt_resolve_accumulated(ctx, desc, &acc, samples_done, (uint8_t*)m.rgb8, (float*)m.f32, (float*)m.var, nullptr);
    });
    });
}

// ---- Adaptive sampling (include/dsrt.h, ADAPTIVE SAMPLING): masked sample sets, the convergence test that makes the masks, the per-pixel resolve, the driver ----
namespace {
int check_adaptive(const char* fn, const DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtAdaptive* ad, bool have_args, bool have_sum, bool have_sq, const void* rgb8,
                   const void* f32, const void* var) {
    if (!ad) return accum_fail(fn, "null argument");
    const void* outputs[3] = {rgb8, f32, var};
    if (int rc = check_sums(fn, ctx, desc, have_args, have_sum, have_sq, nullptr, true, outputs)) return rc;
    if (int rc = check_sample_set(fn, ctx, desc, 0, 1, 1)) return rc;                         // whatever a masked launch refuses of ctx and desc
    if (int rc = check_masked_desc(fn, desc)) return rc;
    const int spp = desc->spp < 1 ? 1 : desc->spp;
    if (ad->passes < 1 || ad->passes > spp || ad->passes > 64) return accum_fail(fn, "passes must be between 1 and min(spp, 64)");
    if (ad->min_passes < 1 || ad->min_passes > ad->passes) return accum_fail(fn, "min_passes must be between 1 and passes");
    if (!(ad->rel_tol >= 0.0f) || !(ad->floor >= 0.0f)) return accum_fail(fn, "rel_tol and floor must be >= 0");
    return DSRT_OK;
}
}  // namespace

int dsrt_render_accumulate_masked(DsrtContext* ctx, const DsrtRenderDesc* desc, int first, int count, int stride, const DsrtAccum* acc, const uint8_t* d_mask,
                                  uint32_t* d_n, void* stream, DsrtStats* stats) {
    return dsrt::guarded("dsrt_render_accumulate_masked", [&]() -> int {
    return accumulate_impl("dsrt_render_accumulate_masked", ctx, desc, first, count, stride, acc, true, d_mask, d_n, stream, stats);
    });
}

int dsrt_render_accumulate_masked_to_host(DsrtContext* ctx, const DsrtRenderDesc* desc, int first, int count, int stride, const DsrtAccum* h_acc, const uint8_t* h_mask,
                                          uint32_t* h_n, DsrtStats* stats) {
    return dsrt::guarded("dsrt_render_accumulate_masked_to_host", [&]() -> int {
    return accumulate_to_host("dsrt_render_accumulate_masked_to_host", ctx, desc, first, count, stride, h_acc, true, h_mask, h_n, stats);
    });
}

int dsrt_select_unconverged(DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtAccum* acc, const uint32_t* d_n, float rel_tol, float floor, uint32_t n_min,
                            uint32_t n_max, uint8_t* d_mask, uint32_t* h_active, void* stream_v) {
    return dsrt::guarded("dsrt_select_unconverged", [&]() -> int {
    int rc = check_sums("dsrt_select_unconverged", ctx, desc, acc && d_n, acc && acc->sum, acc && acc->sum_sq, nullptr, true, nullptr);
    if (rc) return rc;
    if (!d_mask) return accum_fail("dsrt_select_unconverged", "the mask is NULL");
    if (!(rel_tol >= 0.0f) || !(floor >= 0.0f)) return accum_fail("dsrt_select_unconverged", "rel_tol and floor must be >= 0");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t stream = (hipStream_t)stream_v;
    if (h_active && (rc = ctx->active_count.grow(1))) return rc;
    if ((rc = launch_begin(ctx, stream, {{h_active ? ctx->active_count.p : nullptr, sizeof(uint32_t)}}))) return rc;      // behind the context's last launch (into these sums, maybe)
    HIP_TRY(launch_select_unconverged((const unsigned long long*)acc->sum, (const unsigned long long*)acc->sum_sq, d_n, (size_t)desc->width * desc->height, rel_tol, floor,
                                      n_min, n_max, d_mask, h_active ? ctx->active_count.p : nullptr, stream));
    if ((rc = launch_finish(ctx, stream, nullptr)) || !h_active) return rc;       // (the next launch reads the mask: it comes behind this one on any stream)
    HIP_TRY(hipMemcpyAsync(h_active, ctx->active_count.p, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return DSRT_OK;
    });
}

int dsrt_resolve_accumulated_counts(DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtAccum* acc, const uint32_t* d_n, uint8_t* d_rgb8, float* d_f32,
                                    float* d_var_of_mean, void* stream_v) {
    return dsrt::guarded("dsrt_resolve_accumulated_counts", [&]() -> int {
    return resolve_sums("dsrt_resolve_accumulated_counts", ctx, desc, acc, true, 0, d_n, d_rgb8, d_f32, d_var_of_mean, (hipStream_t)stream_v);
    });
}

// The driver: passes of one interleaved sample set each; the first min_passes over every pixel, each later one over the pixels the convergence test left
// active behind the pass before it (one 4-byte readback per pass); then the per-pixel resolve.
int dsrt_render_adaptive(DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtAdaptive* ad, const DsrtAccum* acc, uint32_t* d_n, uint8_t* d_rgb8, float* d_f32,
                         float* d_var_of_mean, void* stream_v, DsrtAdaptiveStats* stats) {
    return dsrt::guarded("dsrt_render_adaptive", [&]() -> int {
    int rc = check_adaptive("dsrt_render_adaptive", ctx, desc, ad, acc && d_n, acc && acc->sum, acc && acc->sum_sq, d_rgb8, d_f32, d_var_of_mean);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t stream = (hipStream_t)stream_v;
    const size_t px = (size_t)desc->width * desc->height;
    if ((rc = ctx->adaptive_mask.grow(px))) return rc;
    const int spp = desc->spp < 1 ? 1 : desc->spp, P = ad->passes;
    DsrtAdaptiveStats local;
    std::memset(&local, 0, sizeof local);
    // a `checked` frame reads every pass's status flags (a synchronisation per pass, as a checked launch with stats has): the first flagged pass ends the
    // frame with DSRT_ERR_DEVICE_FLAG, as the primitive would
    DsrtStats pass_stats;
    DsrtStats* const flags = desc->checked != 0 ? &pass_stats : nullptr;
    uint32_t active = (uint32_t)px;
    for (int p = 0; p < P && active; ++p) {
        const int count = (spp - p + P - 1) / P;                                     // len(range(p, spp, P))
        if (p < ad->min_passes) {
            if ((rc = dsrt_render_accumulate(ctx, desc, p, count, P, acc, stream, flags))) return rc;
            HIP_TRY(launch_add_count(d_n, (uint32_t)count, px, stream));
        } else if ((rc = dsrt_render_accumulate_masked(ctx, desc, p, count, P, acc, ctx->adaptive_mask.p, d_n, stream, flags))) return rc;
        local.active[p] = active;
        local.samples_total += (uint64_t)active * (uint64_t)count;
        local.passes_run = p + 1;
        if (p + 1 >= ad->min_passes && p + 1 < P &&
            (rc = dsrt_select_unconverged(ctx, desc, acc, d_n, ad->rel_tol, ad->floor, 0u, 0xFFFFFFFFu, ctx->adaptive_mask.p, &active, stream))) return rc;
    }
    if ((rc = dsrt_resolve_accumulated_counts(ctx, desc, acc, d_n, d_rgb8, d_f32, d_var_of_mean, stream))) return rc;
    if (stats) *stats = local;
    return DSRT_OK;
    });
}

int dsrt_render_adaptive_to_host(DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtAdaptive* ad, uint32_t* h_n, uint8_t* h_rgb8, float* h_f32, float* h_var_of_mean,
                                 DsrtAdaptiveStats* stats) {
    return dsrt::guarded("dsrt_render_adaptive_to_host", [&]() -> int {
    if (!ctx || !desc) return accum_fail("dsrt_render_adaptive_to_host", "null argument");
    if (int rc = check_adaptive("dsrt_render_adaptive_to_host", ctx, desc, ad, true, true, true, h_rgb8, h_f32, h_var_of_mean)) return rc;   // (the call owns sums and counts)
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t px = (size_t)desc->width * (size_t)desc->height;
    FrameScratch f;                                         // the frame's sums live on the device for the call; the counts come back only if asked for
    int rc;
    if ((rc = f.init(px, true, false))) return rc;
    FrameBuffers h{};
    h.rgb8 = h_rgb8; h.f32 = h_f32; h.var = h_var_of_mean;
    if ((rc = staged_frame_call(h, px, true, [&](const FrameBuffers& m) {
            return dsrt_render_adaptive(ctx, desc, ad, &f.acc, f.n.p, (uint8_t*)m.rgb8, (float*)m.f32, (float*)m.var, nullptr, stats);
        }))) return rc;
    if (h_n) HIP_TRY(hipMemcpy(h_n, f.n.p, px * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return DSRT_OK;
    });
}

// ---- The denoiser (include/dsrt.h, DENOISER; denoise_kernel.hip): prepare, one a-trous launch per iteration, output.  It reads the caller's sums, counts and guides
// and writes the caller's outputs and the context's own seven records per pixel; the render buffers, camera and sun are not touched.
// Temporal accumulation (include/dsrt.h, TEMPORAL ACCUMULATION; temporal_kernel.hip) is the denoiser with the history stage in front of its iterations. ----

// The temporal stage's part of a call (dsrt_denoise_temporal): null for the plain denoiser.
struct TemporalInput { const GPUCamera* prev_camera; const float* prev; float* next; const DsrtTemporal* tp; float* prev_xy; float* weight; };

namespace {
int check_denoise_params(const char* fn, const DsrtDenoise* dn) {
    if (!dn) return accum_fail(fn, "null argument");
    if (dn->iterations < 0 || dn->iterations > 6) return accum_fail(fn, "iterations must be between 0 and 6");
    if (dn->normal_power_log2 < 0 || dn->normal_power_log2 > 8) return accum_fail(fn, "normal_power_log2 must be between 0 and 8");
    if (!(dn->sigma_l > 0.0f) || !(dn->sigma_z > 0.0f) || !(dn->sigma_a > 0.0f)) return accum_fail(fn, "sigma_l, sigma_z and sigma_a must be > 0");
    return DSRT_OK;
}

int check_temporal_params(const char* fn, const DsrtTemporal* tp) {
    if (!tp) return accum_fail(fn, "null argument (DsrtTemporal)");
    if (!(tp->alpha_min >= 0.0f && tp->alpha_min <= 1.0f)) return accum_fail(fn, "alpha_min must be between 0 and 1");
    if (!(tp->normal_cos_min >= -1.0f && tp->normal_cos_min <= 1.0f)) return accum_fail(fn, "normal_cos_min must be between -1 and 1");
    if (!(tp->plane_tol > 0.0f)) return accum_fail(fn, "plane_tol must be > 0");
    if (!(tp->min_support > 0.0f && tp->min_support <= 1.0f)) return accum_fail(fn, "min_support must be > 0 and <= 1");
    return DSRT_OK;
}

// The buffers of a denoiser call, device or host form alike (the outputs as the caller gave them: an output not asked for is null).
static FrameBuffers denoise_buffers(const DsrtAccum& acc, const uint32_t* n, const DsrtDenoiseGuides& g, const TemporalInput* t, const void* rgb8, const void* f32, const void* linear, const void* var) {
    return FrameBuffers{acc.sum, acc.sum_sq, n, g.normal, g.position, g.albedo, g.range, rgb8, f32, linear, var,
                        t ? t->prev : nullptr, t ? t->next : nullptr, t ? t->prev_xy : nullptr, t ? t->weight : nullptr};
}

// Everything dsrt_denoise_accumulated and (with `t`) dsrt_denoise_temporal refuse, before anything is launched or written; the same for the host forms' host pointers.
int check_denoise(const char* fn, const DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtAccum* acc, int samples_done, const uint32_t* n, const DsrtDenoiseGuides* guides,
                  const TemporalInput* t, const DsrtDenoise* dn, const uint8_t* rgb8, const float* f32, const float* linear, const float* var) {
    if (!ctx || !desc || !acc || !guides || !dn) return accum_fail(fn, "null argument");
    if (!acc->sum || !acc->sum_sq) return accum_fail(fn, "DsrtAccum.sum or sum_sq is NULL (the filter is guided by the variance: both are required)");
    if (!guides->normal || !guides->position || !guides->albedo || !guides->range) return accum_fail(fn, "a guide channel is NULL (normal, position, albedo and range are required)");
    if (int rc = check_frame_desc(fn, desc, false, true)) return rc;
    if (!n && samples_done < 2) return accum_fail(fn, "samples_done < 2 (the variance needs two samples; pass per-pixel counts otherwise)");
    if (int rc = check_denoise_params(fn, dn)) return rc;
    if (!rgb8 && !f32 && !linear && !var) return accum_fail(fn, "no output");
    Staged s[kFrameBufferCount];
    frame_table(denoise_buffers(*acc, n, *guides, t, rgb8, f32, linear, var), (size_t)desc->width * desc->height, s);
    if (int rc = check_frame_table(fn, s, 0, kFrameTemporal, "an output range overlaps an input range", "two output ranges overlap", nullptr)) return rc;
    if (!t) return DSRT_OK;
    if ((t->prev_camera != nullptr) != (t->prev != nullptr)) return accum_fail(fn, "the previous camera and the previous history go together: both NULL (first frame) or both given");
    if (!t->next) return accum_fail(fn, "the next history is NULL (it is required)");
    if (int rc = check_temporal_params(fn, t->tp)) return rc;
    return check_frame_table(fn, s, kFrameTemporal, kFrameUpscale, "the next history, prev_xy or weight overlaps an input or the previous history",
                             "the next history, prev_xy or weight overlaps another output", "an output range overlaps the previous history");
}

// dsrt_denoise_accumulated and dsrt_denoise_temporal: the checks, then prepare, the temporal stage if there is one, the iterations, output.
static int denoise_impl(const char* fn, DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtAccum* acc, int samples_done, const uint32_t* d_n, const DsrtDenoiseGuides* guides,
                        const TemporalInput* t, const DsrtDenoise* dn, uint8_t* d_rgb8, float* d_f32, float* d_linear, float* d_var, hipStream_t stream) {
    int rc;
    if ((rc = check_denoise(fn, ctx, desc, acc, samples_done, d_n, guides, t, dn, d_rgb8, d_f32, d_linear, d_var))) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t px = (size_t)desc->width * desc->height;
    // (growing frees the old records: the launch that may still read them has to be over first)
    if (ctx->dn_al.n < px && ctx->done_valid) HIP_TRY(hipEventSynchronize(ctx->done));
    for (int k = 0; k < 2; ++k) if ((rc = ctx->dn_cl[k].grow(px)) || (rc = ctx->dn_vl[k].grow(px))) return rc;
    if ((rc = ctx->dn_nr.grow(px)) || (rc = ctx->dn_xf.grow(px)) || (rc = ctx->dn_al.grow(px))) return rc;
    const DenoiseBuffers b{{ctx->dn_cl[0].p, ctx->dn_cl[1].p}, {ctx->dn_vl[0].p, ctx->dn_vl[1].p}, ctx->dn_nr.p, ctx->dn_xf.p, ctx->dn_al.p};
    if ((rc = launch_begin(ctx, stream, {}))) return rc;                             // the context's last launch (an accumulate into these sums, the G-buffer) comes first
    HIP_TRY(launch_denoise_prepare((const unsigned long long*)acc->sum, (const unsigned long long*)acc->sum_sq, samples_done, d_n, guides->normal, guides->position,
                                   guides->albedo, guides->range, px, b, stream));
    if (t) {
        TemporalArgs a;
        std::memset(&a, 0, sizeof a);
        a.cl = b.cl[0]; a.vl = b.vl[0]; a.nr = b.nr; a.xf = b.xf;
        a.prev = (const float4*)t->prev; a.next = (float4*)t->next; a.prev_xy = t->prev_xy; a.weight = t->weight;
        a.counts = d_n; a.samples_done = samples_done; a.width = desc->width; a.height = desc->height;
        if (t->prev_camera) {
            const GPUCamera& c = *t->prev_camera;
            const DsrtF3 v[7] = {c.origin, c.lower_left_corner, c.horizontal, c.vertical, c.u, c.v, c.w};
            for (int k = 0; k < 7; ++k) { a.cam[3 * k] = v[k].x; a.cam[3 * k + 1] = v[k].y; a.cam[3 * k + 2] = v[k].z; }
        }
        a.alpha_min = t->tp->alpha_min; a.normal_cos_min = t->tp->normal_cos_min; a.plane_tol = t->tp->plane_tol; a.min_support = t->tp->min_support;
        HIP_TRY(launch_temporal(a, stream));
    }
    for (int i = 0; i < dn->iterations; ++i)
        HIP_TRY(launch_denoise_atrous(b, i & 1, desc->width, desc->height, 1 << i, dn->normal_power_log2, dn->sigma_l, dn->sigma_z, dn->sigma_a, stream));
    HIP_TRY(launch_denoise_output(b, dn->iterations & 1, px, inv_gamma_of(*desc), desc->math_mode == 1, d_rgb8, d_f32, d_linear, d_var, stream));
    return launch_finish(ctx, stream, nullptr);                                      // the records are the context's: its next launch on any stream comes behind
}

// Their _to_host forms: the same call on device mirrors of the frame's table, the device finished before the results are copied out.
static int denoise_to_host(const char* fn, DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtAccum* h_acc, int samples_done, const uint32_t* h_n, const DsrtDenoiseGuides* h_guides,
                           const TemporalInput* ht, const DsrtDenoise* dn, uint8_t* h_rgb8, float* h_f32, float* h_linear, float* h_var) {
    if (int rc = check_denoise(fn, ctx, desc, h_acc, samples_done, h_n, h_guides, ht, dn, h_rgb8, h_f32, h_linear, h_var)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    const FrameBuffers h = denoise_buffers(*h_acc, h_n, *h_guides, ht, h_rgb8, h_f32, h_linear, h_var);
    return staged_frame_call(h, (size_t)desc->width * desc->height, true, [&](const FrameBuffers& m) {
        const DsrtAccum acc = accum_of(m);
        const DsrtDenoiseGuides g{(const float*)m.normal, (const float*)m.position, (const float*)m.albedo, (const float*)m.range};
        const TemporalInput t{ht ? ht->prev_camera : nullptr, (const float*)m.history_prev, (float*)m.history_next, ht ? ht->tp : nullptr, (float*)m.prev_xy, (float*)m.weight};
        return denoise_impl(fn, ctx, desc, &acc, samples_done, (const uint32_t*)m.n, &g, ht ? &t : nullptr, dn, (uint8_t*)m.rgb8, (float*)m.f32, (float*)m.linear,
                            (float*)m.var, nullptr);
    });
}

// The convenience forms (dsrt_render_denoised_to_host, and `temporal` dsrt_render_denoised_temporal_to_host): what they refuse; *spp is the frame's samples.
static int check_render_denoised(const char* fn, const DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtDenoise* dn, bool temporal, const DsrtTemporal* tp, bool any_output, int* spp) {
    if (!ctx || !desc) return accum_fail(fn, "null argument");
    if (int rc = check_denoise_params(fn, dn)) return rc;
    if (temporal) if (int rc = check_temporal_params(fn, tp)) return rc;
    if (!any_output) return accum_fail(fn, "no output");
    *spp = desc->spp < 1 ? 1 : desc->spp;
    if (int rc = check_sample_set(fn, ctx, desc, 0, *spp, 1)) return rc;              // DSRT_ERR_NO_SCENE before an upload; rng_mode 1, no shards
    if (*spp < 2) return accum_fail(fn, "spp < 2 (the variance needs two samples)");
    return DSRT_OK;
}

// ... and their three steps on a frame's scratch buffers `f`, the images into mirrors of the host's: desc->spp samples with second moments, the G-buffer of the current
// camera, the filter (with `t`, its history stage: prev_xy is the one temporal output they return).
static int render_denoised_to_host(DsrtContext* ctx, const DsrtRenderDesc* desc, int spp, const FrameScratch& f, const TemporalInput* t, const DsrtDenoise* dn, uint8_t* h_rgb8,
                                   float* h_f32, float* h_linear, float* h_var, float* h_prev_xy, DsrtStats* stats) {
    FrameBuffers h{};
    h.rgb8 = h_rgb8; h.f32 = h_f32; h.linear = h_linear; h.var = h_var; h.prev_xy = h_prev_xy;
    DsrtStats local;
    return staged_frame_call(h, (size_t)desc->width * (size_t)desc->height, true, [&](const FrameBuffers& m) -> int {
        int r;
        if ((r = dsrt_render_accumulate(ctx, desc, 0, spp, 1, &f.acc, nullptr, stats ? stats : &local))) return r;
        if ((r = dsrt_render_gbuffer(ctx, desc, &f.gb, nullptr, nullptr))) return r;
        return t ? dsrt_denoise_temporal(ctx, desc, &f.acc, spp, nullptr, &f.guides, t->prev_camera, t->prev, t->next, t->tp, dn, (uint8_t*)m.rgb8, (float*)m.f32,
                                         (float*)m.linear, (float*)m.var, (float*)m.prev_xy, nullptr, nullptr)
                 : dsrt_denoise_accumulated(ctx, desc, &f.acc, spp, nullptr, &f.guides, dn, (uint8_t*)m.rgb8, (float*)m.f32, (float*)m.linear, (float*)m.var, nullptr);
    });
}
}  // namespace

void dsrt_denoise_defaults(DsrtDenoise* out) {
    if (!out) return;
    out->iterations = 5; out->normal_power_log2 = 5;
    out->sigma_l = 1.0f; out->sigma_z = 0.01f; out->sigma_a = 0.1f;          // sigma_l: 1, not SVGF's 4 (include/dsrt.h says why)
}

void dsrt_temporal_defaults(DsrtTemporal* out) {
    if (!out) return;
    out->alpha_min = 0.1f; out->normal_cos_min = 0.9f; out->plane_tol = 0.01f; out->min_support = 0.9f;      // min_support: 0.9, not one tap of four (include/dsrt.h says why)
}

int dsrt_denoise_accumulated(DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtAccum* acc, int samples_done, const uint32_t* d_n, const DsrtDenoiseGuides* guides,
                             const DsrtDenoise* dn, uint8_t* d_rgb8, float* d_f32, float* d_linear, float* d_var, void* stream_v) {
    return dsrt::guarded("dsrt_denoise_accumulated", [&]() -> int {
    return denoise_impl("dsrt_denoise_accumulated", ctx, desc, acc, samples_done, d_n, guides, nullptr, dn, d_rgb8, d_f32, d_linear, d_var, (hipStream_t)stream_v);
    });
}

int dsrt_denoise_accumulated_to_host(DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtAccum* h_acc, int samples_done, const uint32_t* h_n, const DsrtDenoiseGuides* h_guides,
                                     const DsrtDenoise* dn, uint8_t* h_rgb8, float* h_f32, float* h_linear, float* h_var) {
    return dsrt::guarded("dsrt_denoise_accumulated_to_host", [&]() -> int {
    return denoise_to_host("dsrt_denoise_accumulated_to_host", ctx, desc, h_acc, samples_done, h_n, h_guides, nullptr, dn, h_rgb8, h_f32, h_linear, h_var);
    });
}

int dsrt_denoise_temporal(DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtAccum* acc, int samples_done, const uint32_t* d_n, const DsrtDenoiseGuides* guides,
                          const GPUCamera* prev_camera, const float* d_history_prev, float* d_history_next, const DsrtTemporal* tp, const DsrtDenoise* dn,
                          uint8_t* d_rgb8, float* d_f32, float* d_linear, float* d_var, float* d_prev_xy, float* d_weight, void* stream_v) {
    return dsrt::guarded("dsrt_denoise_temporal", [&]() -> int {
    const TemporalInput t{prev_camera, d_history_prev, d_history_next, tp, d_prev_xy, d_weight};
    return denoise_impl("dsrt_denoise_temporal", ctx, desc, acc, samples_done, d_n, guides, &t, dn, d_rgb8, d_f32, d_linear, d_var, (hipStream_t)stream_v);
    });
}

int dsrt_denoise_temporal_to_host(DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtAccum* h_acc, int samples_done, const uint32_t* h_n, const DsrtDenoiseGuides* h_guides,
                                  const GPUCamera* prev_camera, const float* h_history_prev, float* h_history_next, const DsrtTemporal* tp, const DsrtDenoise* dn,
                                  uint8_t* h_rgb8, float* h_f32, float* h_linear, float* h_var, float* h_prev_xy, float* h_weight) {
    return dsrt::guarded("dsrt_denoise_temporal_to_host", [&]() -> int {
    const TemporalInput ht{prev_camera, h_history_prev, h_history_next, tp, h_prev_xy, h_weight};
    return denoise_to_host("dsrt_denoise_temporal_to_host", ctx, desc, h_acc, samples_done, h_n, h_guides, &ht, dn, h_rgb8, h_f32, h_linear, h_var);
    });
}

// The convenience form: sums and guides live on the device for the call.
int dsrt_render_denoised_to_host(DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtDenoise* dn, uint8_t* h_rgb8, float* h_f32, float* h_linear, float* h_var, DsrtStats* stats) {
    return dsrt::guarded("dsrt_render_denoised_to_host", [&]() -> int {
    int spp, rc;
    if ((rc = check_render_denoised("dsrt_render_denoised_to_host", ctx, desc, dn, false, nullptr, h_rgb8 || h_f32 || h_linear || h_var, &spp))) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    FrameScratch f;
    if ((rc = f.init((size_t)desc->width * (size_t)desc->height, false, true))) return rc;
    return render_denoised_to_host(ctx, desc, spp, f, nullptr, dn, h_rgb8, h_f32, h_linear, h_var, nullptr, stats);
    });
}

// The same with the histories and the previous camera kept by the context from call to call.
int dsrt_render_denoised_temporal_to_host(DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtDenoise* dn, const DsrtTemporal* tp, int reset, uint8_t* h_rgb8, float* h_f32,
                                          float* h_linear, float* h_var, float* h_prev_xy, DsrtStats* stats) {
    return dsrt::guarded("dsrt_render_denoised_temporal_to_host", [&]() -> int {
    int spp, rc;
    if ((rc = check_render_denoised("dsrt_render_denoised_temporal_to_host", ctx, desc, dn, true, tp, h_rgb8 || h_f32 || h_linear || h_var, &spp))) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t px = (size_t)desc->width * (size_t)desc->height;
    const bool fresh = reset != 0 || !ctx->tp_valid || ctx->tp_width != desc->width || ctx->tp_height != desc->height;
    FrameScratch f;
    if ((rc = f.init(px, false, true))) return rc;
    if (fresh) ctx->tp_valid = false;                                                 // (growing does not keep the contents: a sequence of another size is over either way)
    for (DevBuf<float4>& h : ctx->tp_hist) if ((rc = h.grow(px * 4))) return rc;      // (only this call, which is synchronous, uses them: nothing in flight reads them)
    const GPUCamera camera = ctx->frame.camera, prev_camera = ctx->tp_camera;
    const TemporalInput t{fresh ? nullptr : &prev_camera, fresh ? nullptr : (const float*)ctx->tp_hist[ctx->tp_cur].p, (float*)ctx->tp_hist[fresh ? 0 : ctx->tp_cur ^ 1].p, tp,
                          nullptr, nullptr};
    if ((rc = render_denoised_to_host(ctx, desc, spp, f, &t, dn, h_rgb8, h_f32, h_linear, h_var, h_prev_xy, stats))) return rc;
    ctx->tp_cur = fresh ? 0 : ctx->tp_cur ^ 1;
    ctx->tp_camera = camera; ctx->tp_width = desc->width; ctx->tp_height = desc->height;
    ctx->tp_valid = true;
    return DSRT_OK;
    });
}

// ---- The upscaler (include/dsrt.h, UPSCALER; upscale_kernel.hip): pack the low-resolution frame, one launch over the output pixels.  It reads the caller's colour,
// variance and the two rasters' guides and writes the caller's outputs and the context's own five records per low-resolution pixel. ----
namespace {
static int check_upscale_params(const char* fn, const DsrtUpscale* up) {
    if (!up) return accum_fail(fn, "null argument (DsrtUpscale)");
    if (up->normal_power_log2 < 0 || up->normal_power_log2 > 8) return accum_fail(fn, "normal_power_log2 must be between 0 and 8");
    if (!(up->sigma_z > 0.0f) || !(up->sigma_a > 0.0f)) return accum_fail(fn, "sigma_z and sigma_a must be > 0");
    return DSRT_OK;
}

// The buffers of an upscaler call, device or host form alike: the shared rows are the output raster's.
static FrameBuffers upscale_buffers(const float* lo_linear, const float* lo_var, const DsrtUpscaleGuides& lo, const DsrtUpscaleGuides& hi, const void* rgb8, const void* f32,
                                    const void* linear, const void* var, const void* support) {
    FrameBuffers b{};
    b.normal = hi.normal; b.position = hi.position; b.albedo = hi.albedo; b.range = hi.range; b.flags = hi.flags;
    b.rgb8 = rgb8; b.f32 = f32; b.linear = linear; b.var = var; b.support = support;
    b.lo_linear = lo_linear; b.lo_var = lo_var;
    b.lo_normal = lo.normal; b.lo_position = lo.position; b.lo_albedo = lo.albedo; b.lo_range = lo.range; b.lo_flags = lo.flags;
    return b;
}
static DsrtUpscaleGuides lo_guides_of(const FrameBuffers& m) { return DsrtUpscaleGuides{(const float*)m.lo_normal, (const float*)m.lo_position, (const float*)m.lo_albedo, (const float*)m.lo_range, (const uint8_t*)m.lo_flags}; }
static DsrtUpscaleGuides hi_guides_of(const FrameBuffers& m) { return DsrtUpscaleGuides{(const float*)m.normal, (const float*)m.position, (const float*)m.albedo, (const float*)m.range, (const uint8_t*)m.flags}; }

// What of the two rasters' sizes is refused (desc's own is check_frame_desc's).
static int check_upscale_sizes(const char* fn, int lo_width, int lo_height, int width, int height) {
    if (lo_width < 2 || lo_height < 2) return accum_fail(fn, "lo_width and lo_height must be >= 2");
    if (width < lo_width || height < lo_height) return accum_fail(fn, "the output must be at least as large as the low-resolution frame (W >= lo_width, H >= lo_height)");
    return DSRT_OK;
}

// Everything dsrt_upscale_guided refuses, before anything is launched or written; the same for the host form's host pointers.
static int check_upscale(const char* fn, const DsrtContext* ctx, const DsrtRenderDesc* desc, int lo_width, int lo_height, const float* lo_linear, const float* lo_var,
                         const DsrtUpscaleGuides* lo, const DsrtUpscaleGuides* hi, const DsrtUpscale* up, const uint8_t* rgb8, const float* f32, const float* linear,
                         const float* var, const float* support) {
    if (!ctx || !desc || !lo_linear || !lo || !hi || !up) return accum_fail(fn, "null argument");
    for (const DsrtUpscaleGuides* g : {lo, hi})
        if (!g->normal || !g->position || !g->albedo || !g->range) return accum_fail(fn, "a guide channel is NULL (normal, position, albedo and range are required; flags is the optional one)");
    if (int rc = check_frame_desc(fn, desc, false, true)) return rc;
    if (int rc = check_upscale_sizes(fn, lo_width, lo_height, desc->width, desc->height)) return rc;
    if (int rc = check_upscale_params(fn, up)) return rc;
    if (!rgb8 && !f32 && !linear && !var && !support) return accum_fail(fn, "no output");
    if (var && !lo_var) return accum_fail(fn, "the variance output needs the low-resolution variance (d_lo_var)");
    Staged s[kFrameBufferCount];
    frame_table(upscale_buffers(lo_linear, lo_var, *lo, *hi, rgb8, f32, linear, var, support), (size_t)desc->width * desc->height, s, (size_t)lo_width * lo_height);
    return check_frame_table(fn, s, 0, kFrameBufferCount, "an output range overlaps an input range", "two output ranges overlap", nullptr);
}

static int upscale_impl(const char* fn, DsrtContext* ctx, const DsrtRenderDesc* desc, int lo_width, int lo_height, const float* d_lo_linear, const float* d_lo_var,
                        const DsrtUpscaleGuides* lo, const DsrtUpscaleGuides* hi, const DsrtUpscale* up, uint8_t* d_rgb8, float* d_f32, float* d_linear, float* d_var,
                        float* d_support, hipStream_t stream) {
    int rc;
    if ((rc = check_upscale(fn, ctx, desc, lo_width, lo_height, d_lo_linear, d_lo_var, lo, hi, up, d_rgb8, d_f32, d_linear, d_var, d_support))) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t px_lo = (size_t)lo_width * lo_height;
    // (growing frees the old records: the launch that may still read them has to be over first)
    if (ctx->up_rec[4].n < px_lo && ctx->done_valid) HIP_TRY(hipEventSynchronize(ctx->done));
    for (DevBuf<float4>& r : ctx->up_rec) if ((rc = r.grow(px_lo))) return rc;
    const UpscaleRecords rec{ctx->up_rec[0].p, ctx->up_rec[1].p, ctx->up_rec[2].p, ctx->up_rec[3].p, ctx->up_rec[4].p};
    if ((rc = launch_begin(ctx, stream, {}))) return rc;                             // the context's last launch (the denoiser, a G-buffer) comes first
    HIP_TRY(launch_upscale_pack(d_lo_linear, d_lo_var, lo->normal, lo->position, lo->albedo, lo->range, lo->flags, px_lo, rec, stream));
    UpscaleArgs a;
    std::memset(&a, 0, sizeof a);
    a.cr = rec.cr; a.vf = rec.vf; a.nn = rec.nn; a.xx = rec.xx; a.aa = rec.aa;
    a.hi_normal = hi->normal; a.hi_position = hi->position; a.hi_albedo = hi->albedo; a.hi_range = hi->range; a.hi_flags = hi->flags;
    a.out_rgb8 = d_rgb8; a.out_f32 = d_f32; a.out_linear = d_linear; a.out_var = d_var; a.out_support = d_support;
    a.w = lo_width; a.h = lo_height; a.W = desc->width; a.H = desc->height;
    a.normal_power_log2 = up->normal_power_log2; a.use_sun = up->use_sun != 0; a.lo_has_flags = lo->flags != nullptr;
    a.sigma_z = up->sigma_z; a.sigma_a = up->sigma_a; a.inv_gamma = inv_gamma_of(*desc);
    HIP_TRY(launch_upscale(a, desc->math_mode == 1, stream));
    return launch_finish(ctx, stream, nullptr);                                      // the records are the context's: its next launch on any stream comes behind
}
}  // namespace

void dsrt_upscale_defaults(DsrtUpscale* out) {
    if (!out) return;
    out->normal_power_log2 = 5; out->sigma_z = 0.01f; out->sigma_a = 0.1f; out->use_sun = 1;
}

int dsrt_upscale_guided(DsrtContext* ctx, const DsrtRenderDesc* desc, int lo_width, int lo_height, const float* d_lo_linear, const float* d_lo_var, const DsrtUpscaleGuides* lo,
                        const DsrtUpscaleGuides* hi, const DsrtUpscale* up, uint8_t* d_rgb8, float* d_f32, float* d_linear, float* d_var, float* d_support, void* stream_v) {
    return dsrt::guarded("dsrt_upscale_guided", [&]() -> int {
    return upscale_impl("dsrt_upscale_guided", ctx, desc, lo_width, lo_height, d_lo_linear, d_lo_var, lo, hi, up, d_rgb8, d_f32, d_linear, d_var, d_support, (hipStream_t)stream_v);
    });
}

int dsrt_upscale_guided_to_host(DsrtContext* ctx, const DsrtRenderDesc* desc, int lo_width, int lo_height, const float* h_lo_linear, const float* h_lo_var,
                                const DsrtUpscaleGuides* h_lo, const DsrtUpscaleGuides* h_hi, const DsrtUpscale* up, uint8_t* h_rgb8, float* h_f32, float* h_linear, float* h_var,
                                float* h_support) {
    return dsrt::guarded("dsrt_upscale_guided_to_host", [&]() -> int {
    const char* fn = "dsrt_upscale_guided_to_host";
    if (int rc = check_upscale(fn, ctx, desc, lo_width, lo_height, h_lo_linear, h_lo_var, h_lo, h_hi, up, h_rgb8, h_f32, h_linear, h_var, h_support)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    const FrameBuffers h = upscale_buffers(h_lo_linear, h_lo_var, *h_lo, *h_hi, h_rgb8, h_f32, h_linear, h_var, h_support);
    return staged_frame_call(h, (size_t)desc->width * desc->height, true, [&](const FrameBuffers& m) {
        const DsrtUpscaleGuides lo = lo_guides_of(m), hi = hi_guides_of(m);
        return upscale_impl(fn, ctx, desc, lo_width, lo_height, (const float*)m.lo_linear, (const float*)m.lo_var, &lo, &hi, up, (uint8_t*)m.rgb8, (float*)m.f32, (float*)m.linear,
                            (float*)m.var, (float*)m.support, nullptr);
    }, (size_t)lo_width * lo_height);
    });
}

// The convenience form: the five calls of include/dsrt.h, the low-resolution frame and both rasters' guides on the device for the call.
int dsrt_render_upscaled_to_host(DsrtContext* ctx, const DsrtRenderDesc* lo_desc, int out_width, int out_height, const DsrtDenoise* denoise, const DsrtUpscale* up,
                                 uint8_t* h_rgb8, float* h_f32, float* h_linear, float* h_var, uint8_t* h_lo_rgb8, DsrtStats* stats) {
    return dsrt::guarded("dsrt_render_upscaled_to_host", [&]() -> int {
    const char* fn = "dsrt_render_upscaled_to_host";
    DsrtDenoise dn;
    dsrt_denoise_defaults(&dn);
    if (denoise) dn = *denoise; else dn.iterations = 0;
    int spp, rc;
    if (!ctx || !lo_desc) return accum_fail(fn, "null argument");
    DsrtRenderDesc hi_desc = *lo_desc;
    hi_desc.width = out_width; hi_desc.height = out_height;
    if ((rc = check_frame_desc(fn, lo_desc, false, true)) || (rc = check_frame_desc(fn, &hi_desc, false, true))) return rc;
    if ((rc = check_upscale_sizes(fn, lo_desc->width, lo_desc->height, out_width, out_height)) || (rc = check_upscale_params(fn, up))) return rc;
    if ((rc = check_render_denoised(fn, ctx, lo_desc, &dn, false, nullptr, h_rgb8 || h_f32 || h_linear || h_var, &spp))) return rc;      // (the scene is looked for last)
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t px_lo = (size_t)lo_desc->width * (size_t)lo_desc->height, px = (size_t)out_width * (size_t)out_height;
    FrameScratch f, g;                                                    // f: the low-resolution frame's sums and guides; g: the output raster's guides (its sums are not used)
    DevBuf<float> lo_linear, lo_var;
    DevBuf<uint8_t> lo_flags, hi_flags;
    if ((rc = f.init(px_lo, false, true)) || (rc = lo_linear.alloc(px_lo * 3)) || (rc = lo_var.alloc(px_lo * 3)) || (rc = lo_flags.alloc(px_lo))) return rc;
    if ((rc = g.normal.alloc(px * 3)) || (rc = g.position.alloc(px * 3)) || (rc = g.albedo.alloc(px * 3)) || (rc = g.range.alloc(px)) || (rc = hi_flags.alloc(px))) return rc;
    f.gb.flags = lo_flags.p;
    g.gb.normal = g.normal.p; g.gb.position = g.position.p; g.gb.albedo = g.albedo.p; g.gb.range = g.range.p; g.gb.flags = hi_flags.p;
    const DsrtUpscaleGuides lo{f.normal.p, f.position.p, f.albedo.p, f.range.p, lo_flags.p}, hi{g.normal.p, g.position.p, g.albedo.p, g.range.p, hi_flags.p};
    FrameBuffers h{};
    h.rgb8 = h_rgb8; h.f32 = h_f32; h.linear = h_linear; h.var = h_var; h.lo_rgb8 = h_lo_rgb8;
    DsrtStats local;
    return staged_frame_call(h, px, true, [&](const FrameBuffers& m) -> int {
        int r;
        if ((r = dsrt_render_accumulate(ctx, lo_desc, 0, spp, 1, &f.acc, nullptr, stats ? stats : &local))) return r;
        if ((r = dsrt_render_gbuffer(ctx, lo_desc, &f.gb, nullptr, nullptr))) return r;
        if ((r = dsrt_denoise_accumulated(ctx, lo_desc, &f.acc, spp, nullptr, &f.guides, &dn, (uint8_t*)m.lo_rgb8, nullptr, lo_linear.p, lo_var.p, nullptr))) return r;
        if ((r = dsrt_render_gbuffer(ctx, &hi_desc, &g.gb, nullptr, nullptr))) return r;
        return dsrt_upscale_guided(ctx, &hi_desc, lo_desc->width, lo_desc->height, lo_linear.p, lo_var.p, &lo, &hi, up, (uint8_t*)m.rgb8, (float*)m.f32, (float*)m.linear,
                                   (float*)m.var, nullptr, nullptr);
    }, px_lo);
    });
}

// The G-buffer pass (gbuffer_kernel.hip): the context's camera and sun, the reference tree, one launch.  It reads the resident scene and writes the
// caller's buffers and one status word of its own; the context's working buffers, camera and sun are not touched.
int dsrt_render_gbuffer(DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtGBuffer* gb, void* stream_v, DsrtStats* stats) {
    return dsrt::guarded("dsrt_render_gbuffer", [&]() -> int {
    if (!ctx || !desc || !gb) { set_error("dsrt_render_gbuffer: null argument"); return DSRT_ERR_INVALID; }
    if (desc->width < 2 || desc->height < 2) { set_error("dsrt_render_gbuffer: width and height must be at least 2 (the camera divides by W-1 and H-1)"); return DSRT_ERR_INVALID; }
    if (desc->shard_count > 1) { set_error("dsrt_render_gbuffer renders whole images only (shard_count <= 1)"); return DSRT_ERR_INVALID; }
    if ((unsigned long long)desc->width * (unsigned long long)desc->height >= (1ull << 31)) { set_error("dsrt_render_gbuffer: image too large (2^31 pixels)"); return DSRT_ERR_INVALID; }
    const PackedScene* sc = resident_scene(ctx, "dsrt_render_gbuffer");
    if (!sc) return DSRT_ERR_NO_SCENE;
    HIP_TRY(hipSetDevice(ctx->device));
    GBufferArgs a;
    std::memset(&a, 0, sizeof a);
    a.scene = sc->view;
    const GPUCamera& c = ctx->frame.camera;
    pack_camera(c, a.cam);
    a.neg_w[0] = -c.w.x; a.neg_w[1] = -c.w.y; a.neg_w[2] = -c.w.z;
    a.sun_dir[0] = ctx->frame.sun_dir.x; a.sun_dir[1] = ctx->frame.sun_dir.y; a.sun_dir[2] = ctx->frame.sun_dir.z;
    a.sun_enabled = ctx->frame.sun_enabled;
    a.width = desc->width; a.height = desc->height;
    a.tiles_x = (desc->width + 7) / 8;
    const int tiles = a.tiles_x * ((desc->height + 7) / 8);
    a.stack_entries = std::max(1, std::min(64, sc->view.stack_need));       // upload refuses trees that need more than 64
    a.t = gb->t; a.range = gb->range; a.depth = gb->depth; a.position = gb->position; a.normal = gb->normal; a.uv = gb->uv; a.albedo = gb->albedo;
    a.prim_id = gb->prim_id; a.material_id = gb->material_id; a.sun_cos = gb->sun_cos; a.flags = gb->flags;
    if (int rc = ctx->gb_status.grow(1)) return rc;
    a.status = ctx->gb_status.p;
    return launch_enveloped(ctx, (hipStream_t)stream_v, a.status, stats, "G-buffer", tiles, [&](hipStream_t s) { return launch_gbuffer(a, tiles, s); });
    });
}

int dsrt_render_gbuffer_to_host(DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtGBuffer* gb, DsrtStats* stats) {
    return dsrt::guarded("dsrt_render_gbuffer_to_host", [&]() -> int {
    if (!ctx || !desc || !gb) { set_error("dsrt_render_gbuffer_to_host: null argument"); return DSRT_ERR_INVALID; }
    if (desc->width < 2 || desc->height < 2 || desc->shard_count > 1 || (unsigned long long)desc->width * (unsigned long long)desc->height >= (1ull << 31)) {
        set_error("dsrt_render_gbuffer_to_host: bad size or shard"); return DSRT_ERR_INVALID;
    }
    if (!resident_scene(ctx, "dsrt_render_gbuffer_to_host")) return DSRT_ERR_NO_SCENE;
    HIP_TRY(hipSetDevice(ctx->device));
    Staged s[11];
    channels(*gb, kGBufferBytes, (size_t)desc->width * desc->height, Dir::Out, s);
    DsrtStats local;
    return staged_call(s, [&](void* const* d) {
        const DsrtGBuffer dg = pointers_as<DsrtGBuffer>(d);
        return dsrt_render_gbuffer(ctx, desc, &dg, nullptr, stats ? stats : &local);
    });
    });
}

int dsrt_trace_rays(DsrtContext* ctx, int count, const DsrtRays* rays, int mode, const DsrtRayHits* hits, void* stream_v, DsrtStats* stats) {
    return dsrt::guarded("dsrt_trace_rays", [&]() -> int {
    if (int rc = check_trace_args("dsrt_trace_rays", ctx, count, rays, mode, hits)) return rc;
    const PackedScene* sc = resident_scene(ctx, "dsrt_trace_rays");
    if (!sc) return DSRT_ERR_NO_SCENE;
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (count == 0) return DSRT_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const bool any_hit = mode == DSRT_TRACE_ANY;
    RaycastArgs a;
    std::memset(&a, 0, sizeof a);
    a.scene = sc->view;
    a.origins = rays->origins; a.dirs = rays->dirs; a.t_min = rays->t_min; a.t_max = rays->t_max;
    a.count = count;
    a.stack_entries = std::max(1, std::min(64, sc->view.stack_need));       // upload refuses trees that need more than 64
    a.t = hits->t; a.range = hits->range; a.position = hits->position; a.normal = hits->normal; a.uv = hits->uv; a.albedo = hits->albedo;
    a.prim_id = hits->prim_id; a.material_id = hits->material_id; a.flags = hits->flags;
    if (int rc = ctx->rc_status.grow(1)) return rc;
    a.status = ctx->rc_status.p;
    const int blocks = (int)(((size_t)count + 63) / 64);                   // one lane per ray
    return launch_enveloped(ctx, (hipStream_t)stream_v, a.status, stats, "ray query", blocks, [&](hipStream_t s) { return launch_raycast(a, any_hit, blocks, s); });
    });
}

int dsrt_trace_rays_to_host(DsrtContext* ctx, int count, const DsrtRays* rays, int mode, const DsrtRayHits* hits, DsrtStats* stats) {
    return dsrt::guarded("dsrt_trace_rays_to_host", [&]() -> int {
    if (int rc = check_trace_args("dsrt_trace_rays_to_host", ctx, count, rays, mode, hits)) return rc;
    if (!resident_scene(ctx, "dsrt_trace_rays_to_host")) return DSRT_ERR_NO_SCENE;
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (count == 0) return DSRT_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    Staged s[4 + 9];
    channels(*rays, kRayBytes, (size_t)count, Dir::In, s);
    channels(*hits, kRayHitBytes, (size_t)count, Dir::Out, s + 4);
    DsrtStats local;
    return staged_call(s, [&](void* const* d) {
        const DsrtRays dr = pointers_as<DsrtRays>(d);
        const DsrtRayHits dh = pointers_as<DsrtRayHits>(d + 4);
        return dsrt_trace_rays(ctx, count, &dr, mode, &dh, nullptr, stats ? stats : &local);
    });
    });
}

int dsrt_selftest_poke_node_word(DsrtContext* ctx, size_t word_index, uint32_t value, uint32_t* old_value) {
    if (!resident_scene(ctx, "dsrt_selftest_poke_node_word")) return DSRT_ERR_NO_SCENE;
    if (word_index >= ctx->scene->pairs.n * 4) { set_error("dsrt_selftest_poke_node_word: word index beyond the node records"); return DSRT_ERR_INVALID; }
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipDeviceSynchronize());
    uint32_t* w = reinterpret_cast<uint32_t*>(ctx->scene->pairs.p) + word_index;
    if (old_value) HIP_TRY(hipMemcpy(old_value, w, 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(w, &value, 4, hipMemcpyHostToDevice));
    return DSRT_OK;
}

int dsrt_selftest_read_scene_words(DsrtContext* ctx, int array, size_t first_word, size_t n_words, uint32_t* out) {
    if (!resident_scene(ctx, "dsrt_selftest_read_scene_words")) return DSRT_ERR_NO_SCENE;
    const PackedScene& sc = *ctx->scene;
    if (array < 0 || array > 2) { set_error("dsrt_selftest_read_scene_words: no such array"); return DSRT_ERR_INVALID; }
    const DevBuf<float4>& buf = array == 0 ? sc.pairs : array == 1 ? sc.tri_pairs : sc.tri_shade;
    const size_t words = buf.n * 4;
    if (first_word > words || n_words > words - first_word) { set_error("dsrt_selftest_read_scene_words: range beyond the array"); return DSRT_ERR_INVALID; }
    if (!out || !n_words) return DSRT_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, reinterpret_cast<const uint32_t*>(buf.p) + first_word, n_words * 4, hipMemcpyDeviceToHost));
    return DSRT_OK;
}

int dsrt_selftest_math(DsrtContext* ctx, int fn, const float* x, float y, float* out, int n) {
    if (!ctx || !x || !out || n <= 0 || fn < 0 || fn > 2) { set_error("dsrt_selftest_math: bad argument"); return DSRT_ERR_INVALID; }
    HIP_TRY(hipSetDevice(ctx->device));
    DevBuf<float> dx, dy;
    int rc;
    if ((rc = dx.alloc((size_t)n)) || (rc = dy.alloc((size_t)n))) return rc;
    HIP_TRY(hipMemcpy(dx.p, x, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(launch_math(fn, dx.p, y, dy.p, n, nullptr));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, dy.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return DSRT_OK;
}

int dsrt_selftest_devkat(DsrtContext* ctx, int fn, const float* in12, float* out12, int n) {
    if (!ctx || !in12 || !out12 || n <= 0 || fn < 0 || fn > 5) { set_error("dsrt_selftest_devkat: bad argument"); return DSRT_ERR_INVALID; }
    HIP_TRY(hipSetDevice(ctx->device));
    DevBuf<float> di, dout;
    int rc;
    if ((rc = di.alloc((size_t)n * 12)) || (rc = dout.alloc((size_t)n * 12))) return rc;
    HIP_TRY(hipMemcpy(di.p, in12, (size_t)n * 12 * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(dout.p, 0, (size_t)n * 12 * sizeof(float)));
    HIP_TRY(launch_devkat(fn, di.p, dout.p, n, nullptr));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out12, dout.p, (size_t)n * 12 * sizeof(float), hipMemcpyDeviceToHost));
    return DSRT_OK;
}

int dsrt_selftest_philox(DsrtContext* ctx, uint64_t seed, uint64_t subsequence, int n, uint32_t* ours, uint32_t* rocrand_words) {
    if (!ctx || !ours || !rocrand_words || n <= 0) { set_error("dsrt_selftest_philox: bad argument"); return DSRT_ERR_INVALID; }
    HIP_TRY(hipSetDevice(ctx->device));
    DevBuf<uint32_t> a, b;
    int rc;
    if ((rc = a.alloc((size_t)n)) || (rc = b.alloc((size_t)n))) return rc;
    HIP_TRY(launch_philox(seed, subsequence, n, a.p, b.p, nullptr));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(ours, a.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(rocrand_words, b.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return DSRT_OK;
}

// =========================================================================================
// Drop-in layer
// =========================================================================================
static void gpu_render_scene_body(const GPUScene* scene, int width, int height);
namespace {
std::mutex g_dropin_mutex;
DsrtContext* g_dropin_ctx = nullptr;

// The reference calls build_gpu_scene + gpu_render_scene + free_gpu_scene once per FRAME (src/main.cpp:405-428) although only camera
// and sun change between frames.  gpu_render_scene receives device arrays in the reference layouts; converting them (copy to the
// host, re-layout, upload) costs far more than rendering a far frame.  So the drop-in keeps the converted scene of the previous call
// and re-uses it when the arrays it is handed have the same CONTENT: a 128-bit position-dependent hash of every array, computed on
// the device (one pass over ~150 MB at 1 M triangles: well under a millisecond), plus all the counts.  Pointer equality would not do --
// the reference frees and re-allocates the arrays every frame, so equal pointers can hold different data and vice versa.
struct SceneFingerprint {
    uint64_t h[2] = {0, 0};
    int counts[7] = {0, 0, 0, 0, 0, 0, 0};
    bool valid = false;
    bool operator==(const SceneFingerprint& o) const { return valid && o.valid && h[0] == o.h[0] && h[1] == o.h[1] && !std::memcmp(counts, o.counts, sizeof counts); }
};
SceneFingerprint g_dropin_fp;
// two words of device memory for the hash; like g_dropin_ctx a raw pointer that is never freed: a destructor at static-destruction time
// would call hipFree after the HIP runtime may already be gone
uint64_t* g_dropin_hash = nullptr;

int fingerprint_device_scene(const GPUScene& d, SceneFingerprint& fp) {
    fp = SceneFingerprint{};
    const int counts[7] = {d.num_triangles, d.num_spheres, d.num_materials, d.num_bvh_nodes, d.num_textures, d.texture_pool_floats, d.tri_indices ? 1 : 0};
    std::memcpy(fp.counts, counts, sizeof counts);
    for (int c : counts) if (c < 0) { set_error("scene has a negative count"); return DSRT_ERR_INVALID; }
    if (!g_dropin_hash) HIP_TRY(hipMalloc((void**)&g_dropin_hash, 2 * sizeof(uint64_t)));
    HIP_TRY(hipMemsetAsync(g_dropin_hash, 0, 2 * sizeof(uint64_t), nullptr));
    int k = 0;                                                             // every array's salt: its place in the walk
    const int rc = for_each_scene_array(d, [&](const auto* p, size_t n) -> int {
        ++k;
        if (n) HIP_TRY(launch_content_hash((const uint32_t*)p, n * sizeof(*p) / 4, 0x9E3779B97F4A7C15ull * (uint64_t)k, g_dropin_hash, nullptr));
        return DSRT_OK;
    });
    if (rc) return rc;
    HIP_TRY(hipMemcpy(fp.h, g_dropin_hash, sizeof fp.h, hipMemcpyDeviceToHost));
    fp.valid = true;
    return DSRT_OK;
}

DsrtContext* dropin_context() {
    if (!g_dropin_ctx) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) dev = 0;
        if (dsrt_ctx_create(dev, &g_dropin_ctx) != DSRT_OK) return nullptr;
    }
    return g_dropin_ctx;
}
}  // namespace

int dsrt_dropin_has_certified_tree(void) {
    std::lock_guard<std::mutex> lock(g_dropin_mutex);
    return dsrt_ctx_has_certified_tree(g_dropin_ctx);
}

int dsrt_build_gpu_scene(const DsrtHostScene* hs, const GPUCamera* cam, const float sun_dir_model[3], GPUScene* out) {
    return dsrt::guarded("dsrt_build_gpu_scene", [&]() -> int {
    if (!hs || !cam || !out) { set_error("dsrt_build_gpu_scene: null argument"); return DSRT_ERR_INVALID; }
    GPUScene h;
    int rc = dsrt_host_scene_view(hs, &h);
    if (rc) return rc;
    dsrt_scene_set_frame(&h, cam, sun_dir_model);
    // The returned header carries DEVICE arrays in the reference layouts, like the reference's own builder.  A failure frees what was pushed before it
    // and leaves *out as it was.
    GPUScene d = h;
    void* pushed[kSceneArrays];
    size_t n_pushed = 0;
    rc = for_each_scene_array(d, [&](auto*& p, size_t n) -> int {
        const void* src = p;
        p = nullptr;
        if (!n) return DSRT_OK;
        HIP_TRY(hipMalloc((void**)&p, n * sizeof(*p)));
        assert(n_pushed < kSceneArrays);
        pushed[n_pushed++] = (void*)p;
        HIP_TRY(hipMemcpy((void*)p, src, n * sizeof(*p), hipMemcpyHostToDevice));
        return DSRT_OK;
    });
    if (rc) { while (n_pushed) (void)hipFree(pushed[--n_pushed]); return rc; }
    *out = d;
    return DSRT_OK;
    });
}

void dsrt_free_gpu_scene(GPUScene* s) {                                  // src/gpu_scene_builder.cpp:603-626
    if (!s) return;
    for_each_scene_array(*s, [](auto*& p, size_t) -> int { if (p) (void)hipFree((void*)p); p = nullptr; return DSRT_OK; });
    s->num_triangles = s->num_spheres = s->num_materials = s->num_bvh_nodes = s->num_textures = s->texture_pool_floats = 0;
}

void gpu_render_scene(const GPUScene* scene, int width, int height) {
    (void)dsrt::guarded("gpu_render_scene", [&]() -> int { gpu_render_scene_body(scene, width, height); return DSRT_OK; });
}

static void gpu_render_scene_body(const GPUScene* scene, int width, int height) {
    std::lock_guard<std::mutex> lock(g_dropin_mutex);
    if (!scene) { std::fprintf(stderr, "gpu_render_scene: null scene\n"); return; }
    DsrtContext* ctx = dropin_context();
    if (!ctx) { std::fprintf(stderr, "gpu_render_scene: %s\n", dsrt_last_error()); return; }
    SceneFingerprint fp;
    if (fingerprint_device_scene(*scene, fp) != DSRT_OK) { std::fprintf(stderr, "gpu_render_scene: %s\n", dsrt_last_error()); return; }
    // The reference's entry point has nowhere to ask for the certified second tree either: DSRT_CERTIFIED_TREE=1, looked at on every call here (the one context of the
    // drop-in lives as long as the process); a change of the variable re-converts the scene.
    { const char* e = std::getenv("DSRT_CERTIFIED_TREE"); ctx->want_second_tree = e && e[0] == '1'; }
    if (scene_of(ctx) && fp == g_dropin_fp && ctx->scene->has_second_tree == (ctx->want_second_tree && ctx->scene->view.root_ref != kRefNone)) {
        // same geometry, materials and textures as the previous call: only the per-frame part of the header is taken over
        ctx->frame = frame_of(*scene);
    } else {
        g_dropin_fp.valid = false;
        if (dsrt_scene_upload_device(ctx, scene) != DSRT_OK) { std::fprintf(stderr, "gpu_render_scene: scene upload failed: %s\n", dsrt_last_error()); return; }
        g_dropin_fp = fp;
    }
    DsrtRenderDesc d;
    std::memset(&d, 0, sizeof d);
    d.width = width; d.height = height;
    d.spp = scene->params.samples_per_pixel;
    d.max_depth = scene->params.max_depth;
    d.gamma = scene->params.gamma;
    d.seed = scene->seed;
    d.rng_mode = scene->params.rng_mode == 1 ? 1 : 0;        // the reference always stores 0 here (src/gpu_scene_builder.cpp:577)
    // The reference's entry point has nowhere to say which sinf / cosf / powf (DsrtRenderDesc.math_mode): the environment variable DSRT_MATH_MODE=1 asks this
    // drop-in for the device math library's, i.e. for the very file the reference's own gpu_render_scene writes on this GPU (tests/test_gpu_reference_kernel.py)
    { const char* e = std::getenv("DSRT_MATH_MODE"); d.math_mode = e && std::atoi(e) == 1 ? 1 : 0; }
    std::vector<uint8_t> fb((size_t)width * height * 3);
    if (dsrt_render_to_host(ctx, &d, fb.data(), nullptr, nullptr) != DSRT_OK) { std::fprintf(stderr, "render_kernel failed: %s\n", dsrt_last_error()); return; }
    if (dsrt_write_ppm("image_gpu.ppm", fb.data(), width, height) != DSRT_OK) std::fprintf(stderr, "Failed to open image_gpu.ppm for writing\n");
}

}  // extern "C"

// C++ forms of the reference's builder entry points (declared in host/scene_model.hpp).
namespace dsrt {

GPUScene build_gpu_scene(const hittable_list& world, const camera& cam, const vec3& sun_dir_model) {
    GPUScene out;
    std::memset(&out, 0, sizeof out);
    DsrtHostScene* hs = dsrt_host_scene_create();
    const float sun[3] = {sun_dir_model.x(), sun_dir_model.y(), sun_dir_model.z()};
    const GPUCamera gc = cam.toGPUCamera();
    if (flatten_world(world, hs) != DSRT_OK || dsrt_host_scene_build_bvh(hs) != DSRT_OK || dsrt_build_gpu_scene(hs, &gc, sun, &out) != DSRT_OK)
        std::fprintf(stderr, "build_gpu_scene: %s\n", dsrt_last_error());
    dsrt_host_scene_destroy(hs);
    return out;
}

void free_gpu_scene(GPUScene& scene) { dsrt_free_gpu_scene(&scene); }

}  // namespace dsrt
