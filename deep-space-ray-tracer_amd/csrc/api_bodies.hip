// api_bodies.hip -- movable rigid bodies (include/dsrt.h, MOVABLE RIGID BODIES): what an upload with bodies keeps resident beside the scene (build_bodies),
// and the pose update.  Calls scene_pack.hip (install_scene, which calls build_bodies back) and the launchers of bodies_kernel.hip.
#include <algorithm>
#include <cmath>

#include "api_internal.h"

using namespace dsrt;

static_assert(kMaxBodies == DSRT_MAX_BODIES, "launchers.h and include/dsrt.h disagree on the number of bodies");

// What a pose update needs resident, from the host scene's bodies tree and from where pack_tree put its nodes and triangles.
int dsrt::build_bodies(const DsrtHostScene& hs, const PackReport& rep, PackedScene& sc) {
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
    std::memcpy(bd->host_poses, poses.data(), sizeof bd->host_poses);
    for (int b = 0; b < B; ++b) {
        bd->first_tri.push_back(hs.body_start[b]);
        bd->num_tris.push_back((b + 1 < B ? hs.body_start[b + 1] : N) - hs.body_start[b]);
    }
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

extern "C" {

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
    std::memcpy(bd.host_poses + 12 * (size_t)first_body, poses, 12 * (size_t)count * sizeof(float));
    if (!ctx->tp_bodies) ctx->tp_valid = false;    // the temporal history assumed the scene as it was, unless the sequence follows the bodies (dsrt_ctx_set_temporal_bodies)
    if (ms) {
        for (int i = 0; i < 3; ++i) HIP_TRY(hipEventElapsedTime(&bd.last_ms[i], bd.ev[i], bd.ev[i + 1]));
        HIP_TRY(hipEventElapsedTime(ms, bd.ev[0], bd.ev[3]));
    }
    return DSRT_OK;
}

}  // extern "C"
