// scene_pack.hip -- the scene packer: reference-layout arrays on the host into the traversal layout of device_layout.h, uploaded (pack_tree, pack_scene), and
// install_scene, which makes the result a context's resident scene.  Calls host/bvh_sah.cpp (prepare_second_tree) and api_bodies.hip (build_bodies);
// called by the upload entry points of api_context.hip and api_bodies.hip.
#include <algorithm>
#include <cstdlib>

#include "api_internal.h"

using namespace dsrt;

namespace {

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

// A fresh PackedScene for this context (clones made earlier keep the one they share until they are re-cloned or destroyed).
// `bodies`: the host scene with the bodies tree that `host_layout` views (dsrt_scene_upload_bodies): no second tree, and the resident data of a pose update.
int dsrt::install_scene(DsrtContext* ctx, const GPUScene& host_layout, const DsrtHostScene* bodies) {
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
