// bodies_sanitize_driver.cpp -- test infrastructure (tests/test_bodies_host.py): the host side of movable rigid bodies (host/bvh_bodies.cpp and what it shares with the
// other builders) driven through its C ABI in a build with AddressSanitizer and UndefinedBehaviorSanitizer.  begin / build / pose on: a scene shaped like the
// tests' (a panel, a box, a three-triangle body, a nine-triangle big leaf), a one-triangle body, an empty body 0, 15 bodies (and the refused 16th), empty bodies in
// the middle, and hostile arguments -- which must be refused with the scene's arrays unchanged.  No GPU, no HIP: only deep-space-ray-tracer_amd/host/*.cpp is linked.
//
// usage: bodies_sanitize_driver       exit code 0 = every expectation held
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../include/dsrt.h"

static int g_failures = 0;
#define EXPECT(cond, what) do { if (!(cond)) { std::fprintf(stderr, "FAILED line %d: %s (%s)\n", __LINE__, what, dsrt_last_error()); ++g_failures; } } while (0)

static GPUMaterial grey() { GPUMaterial m; std::memset(&m, 0, sizeof m); m.albedo_tex = -1; m.albedo = DsrtF3{0.7f, 0.7f, 0.7f}; m.ref_idx = 1.5f; return m; }

static GPUTriangle tri(float ax, float ay, float az, float bx, float by, float bz, float cx, float cy, float cz) {
    GPUTriangle t; std::memset(&t, 0, sizeof t);
    t.v0 = DsrtF3{ax, ay, az}; t.v1 = DsrtF3{bx, by, bz}; t.v2 = DsrtF3{cx, cy, cz};
    t.n0 = t.n1 = t.n2 = DsrtF3{0.0f, 0.0f, 1.0f};
    t.albedo_tex = -1;
    return t;
}

// nu x nv quads in the plane z = z0 from (x0, y0), step s
static std::vector<GPUTriangle> grid(float x0, float y0, float z0, float s, int nu, int nv) {
    std::vector<GPUTriangle> out;
    for (int i = 0; i < nu; ++i)
        for (int j = 0; j < nv; ++j) {
            const float x = x0 + s * i, y = y0 + s * j;
            out.push_back(tri(x, y, z0, x + s, y, z0, x + s, y + s, z0));
            out.push_back(tri(x, y, z0, x + s, y + s, z0, x, y + s, z0 + 0.25f * (float)((i + j) % 3)));
        }
    return out;
}

static void add(DsrtHostScene* hs, const std::vector<GPUTriangle>& t) {
    const GPUMaterial m = grey();
    EXPECT(dsrt_host_scene_add_arrays(hs, t.data(), (int)t.size(), nullptr, 0, &m, 1) == DSRT_OK, "add_arrays");
}

struct Snapshot { std::vector<uint8_t> tris, nodes, idx; };
static Snapshot snapshot(const DsrtHostScene* hs) {
    GPUScene v;
    Snapshot s;
    if (dsrt_host_scene_view(hs, &v) != DSRT_OK) return s;
    s.tris.assign((const uint8_t*)v.triangles, (const uint8_t*)v.triangles + sizeof(GPUTriangle) * (size_t)v.num_triangles);
    s.nodes.assign((const uint8_t*)v.bvh_nodes, (const uint8_t*)v.bvh_nodes + sizeof(GPUBVHNode) * (size_t)v.num_bvh_nodes);
    if (v.tri_indices) s.idx.assign((const uint8_t*)v.tri_indices, (const uint8_t*)v.tri_indices + sizeof(int) * (size_t)v.num_triangles);
    return s;
}
static bool same(const Snapshot& a, const Snapshot& b) { return a.tris == b.tris && a.nodes == b.nodes && a.idx == b.idx; }

static void pose(float* p, float angle, float tx, float ty, float tz) {
    const float c = std::cos(angle), s = std::sin(angle);
    const float m[12] = {c, -s, 0, tx, s, c, 0, ty, 0, 0, 1, tz};
    std::memcpy(p, m, sizeof m);
}

// every node reachable once, children inside parents, every triangle under exactly one leaf
static void check_tree(const DsrtHostScene* hs, const char* what) {
    GPUScene v;
    EXPECT(dsrt_host_scene_view(hs, &v) == DSRT_OK, what);
    if (v.num_triangles == 0) { EXPECT(v.num_bvh_nodes == 0, what); return; }
    std::vector<int> seen((size_t)v.num_bvh_nodes, 0), covered((size_t)v.num_triangles, 0), todo{0};
    while (!todo.empty()) {
        const int n = todo.back(); todo.pop_back();
        if (n < 0 || n >= v.num_bvh_nodes || seen[n]++) { EXPECT(false, what); return; }
        const GPUBVHNode& nd = v.bvh_nodes[n];
        if (nd.tri_count > 0) {
            for (int i = 0; i < nd.tri_count; ++i) covered[(size_t)v.tri_indices[nd.tri_offset + i]]++;
        } else {
            for (int c : {nd.left, nd.right}) {
                if (c <= n || c >= v.num_bvh_nodes) { EXPECT(false, "pre-order children"); return; }
                const GPUBVHNode& ch = v.bvh_nodes[c];
                EXPECT(ch.bbox_min.x >= nd.bbox_min.x && ch.bbox_min.y >= nd.bbox_min.y && ch.bbox_min.z >= nd.bbox_min.z &&
                       ch.bbox_max.x <= nd.bbox_max.x && ch.bbox_max.y <= nd.bbox_max.y && ch.bbox_max.z <= nd.bbox_max.z, "child box inside its parent's");
                todo.push_back(c);
            }
        }
    }
    for (int s : seen) EXPECT(s == 1, "every node reached once");
    for (int c : covered) EXPECT(c == 1, "every triangle under one leaf");
}

static void pose_all_and_check(DsrtHostScene* hs, const char* what) {
    const int B = dsrt_host_scene_body_count(hs);
    std::vector<float> p(12 * (size_t)B);
    for (int b = 1; b < B; ++b) pose(&p[12 * (size_t)(b - 1)], 0.37f * (float)b, 1.5f * (float)b, -0.75f * (float)b, 0.125f * (float)b);
    if (B > 1) EXPECT(dsrt_host_scene_set_body_poses(hs, 1, B - 1, p.data()) == DSRT_OK, what);
    check_tree(hs, what);
    if (B > 2) EXPECT(dsrt_host_scene_set_body_poses(hs, B - 1, 1, p.data()) == DSRT_OK, "one body alone");
    check_tree(hs, what);
}

static void hostile(DsrtHostScene* hs) {
    const int B = dsrt_host_scene_body_count(hs);
    std::vector<float> p(12 * (size_t)DSRT_MAX_BODIES, 0.0f);
    for (int b = 0; b < DSRT_MAX_BODIES; ++b) pose(&p[12 * (size_t)b], 0.1f, 0, 0, 0);
    const Snapshot before = snapshot(hs);
    EXPECT(dsrt_host_scene_set_body_poses(hs, 0, 1, p.data()) == DSRT_ERR_INVALID, "body 0 does not move");
    EXPECT(dsrt_host_scene_set_body_poses(hs, B, 1, p.data()) == DSRT_ERR_INVALID, "body past the last");
    EXPECT(dsrt_host_scene_set_body_poses(hs, 1, B, p.data()) == DSRT_ERR_INVALID, "count past the last");
    EXPECT(dsrt_host_scene_set_body_poses(hs, -3, 2, p.data()) == DSRT_ERR_INVALID, "negative body");
    EXPECT(dsrt_host_scene_set_body_poses(hs, 1, -1, p.data()) == DSRT_ERR_INVALID, "negative count");
    EXPECT(dsrt_host_scene_set_body_poses(hs, 1, std::numeric_limits<int>::max(), p.data()) == DSRT_ERR_INVALID, "count that overflows");
    EXPECT(dsrt_host_scene_set_body_poses(hs, std::numeric_limits<int>::max(), std::numeric_limits<int>::max(), p.data()) == DSRT_ERR_INVALID, "both overflow");
    if (B > 1) {
        EXPECT(dsrt_host_scene_set_body_poses(hs, 1, 1, nullptr) == DSRT_ERR_INVALID, "null poses");
        for (float bad : {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity()}) {
            std::vector<float> q = p;
            q[12 * (size_t)(B - 2) + 7] = bad;                       // in the LAST posed body: nothing before it may have been applied
            EXPECT(dsrt_host_scene_set_body_poses(hs, 1, B - 1, q.data()) == DSRT_ERR_INVALID, "non-finite pose entry");
        }
    }
    EXPECT(dsrt_host_scene_set_body_poses(nullptr, 1, 1, p.data()) == DSRT_ERR_INVALID, "null scene");
    EXPECT(same(before, snapshot(hs)), "a refused call changed the scene");
    int first = -1, n = -1;
    EXPECT(dsrt_host_scene_body_range(hs, B, &first, &n) == DSRT_ERR_INVALID && dsrt_host_scene_body_range(hs, -1, &first, &n) == DSRT_ERR_INVALID, "body_range of no body");
    EXPECT(dsrt_host_scene_body_range(nullptr, 0, &first, &n) == DSRT_ERR_INVALID && dsrt_host_scene_body_count(nullptr) == 0, "null scene queries");
    EXPECT(dsrt_host_scene_body_range(hs, 0, nullptr, nullptr) == DSRT_OK, "null outputs are optional");
}

int main() {
    {   // the shape of the tests' scene
        DsrtHostScene* hs = dsrt_host_scene_create();
        add(hs, grid(-6, -6, 0, 1, 12, 12));
        EXPECT(dsrt_host_scene_begin_body(hs) == 1, "body 1");
        add(hs, grid(7, -1, 2, 0.25f, 8, 8));
        EXPECT(dsrt_host_scene_begin_body(hs) == 2, "body 2");
        add(hs, {tri(0, 0, 3, 1, 0, 3, 1, 1, 3), tri(0, 0, 3, 1, 1, 3, 0, 1, 3), tri(0, 0, 3.5f, 1, 0, 3.5f, 0, 1, 3.5f)});
        EXPECT(dsrt_host_scene_begin_body(hs) == 3, "body 3");
        std::vector<GPUTriangle> nine;
        for (int k = 0; k < 9; ++k) {
            const float ax = 0.25f * (float)(k + 1), ay = 0.5f, bx = -0.5f, by = 0.25f * (float)(k + 2);
            nine.push_back(tri(-9 + ax, -8 + ay, 4, -9 + bx, -8 + by, 4, -9 - ax - bx, -8 - ay - by, 4));
        }
        add(hs, nine);
        const float one[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
        EXPECT(dsrt_host_scene_set_body_poses(hs, 1, 1, one) == DSRT_ERR_INVALID, "posing before any tree");
        EXPECT(dsrt_host_scene_build_bvh(hs) == DSRT_OK, "the median builder on a scene with bodies");
        EXPECT(dsrt_host_scene_set_body_poses(hs, 1, 1, one) == DSRT_ERR_INVALID, "posing on the median tree");
        EXPECT(dsrt_host_scene_build_bvh_sah(hs) == DSRT_OK, "the SAH builder on a scene with bodies");
        EXPECT(dsrt_host_scene_set_body_poses(hs, 1, 1, one) == DSRT_ERR_INVALID, "posing on the SAH tree");
        EXPECT(dsrt_host_scene_build_bvh_bodies(hs) == DSRT_OK, "bodies tree");
        EXPECT(dsrt_host_scene_body_count(hs) == 4, "four bodies");
        check_tree(hs, "rest");
        pose_all_and_check(hs, "posed");
        hostile(hs);
        add(hs, {tri(0, 0, 9, 1, 0, 9, 0, 1, 9)});                   // an add after the build: the tree is void, posing refused until it is rebuilt
        EXPECT(dsrt_host_scene_set_body_poses(hs, 1, 1, one) == DSRT_ERR_INVALID, "posing after an add");
        EXPECT(dsrt_host_scene_build_bvh_bodies(hs) == DSRT_OK, "rebuild");
        pose_all_and_check(hs, "posed after the rebuild");
        dsrt_host_scene_destroy(hs);
    }
    {   // a one-triangle body, alone with a static part, and as the only non-empty body
        DsrtHostScene* hs = dsrt_host_scene_create();
        add(hs, grid(0, 0, 0, 1, 3, 3));
        EXPECT(dsrt_host_scene_begin_body(hs) == 1, "body 1");
        add(hs, {tri(0, 0, 1, 1, 0, 1, 0, 1, 1)});
        EXPECT(dsrt_host_scene_build_bvh_bodies(hs) == DSRT_OK, "bodies tree");
        pose_all_and_check(hs, "one-triangle body");
        hostile(hs);
        dsrt_host_scene_destroy(hs);
    }
    {   // an empty body 0 -- and nothing but one movable triangle: no top node at all
        DsrtHostScene* hs = dsrt_host_scene_create();
        EXPECT(dsrt_host_scene_begin_body(hs) == 1, "body 1");
        add(hs, {tri(0, 0, 1, 1, 0, 1, 0, 1, 1)});
        EXPECT(dsrt_host_scene_build_bvh_bodies(hs) == DSRT_OK, "bodies tree");
        GPUScene v;
        EXPECT(dsrt_host_scene_view(hs, &v) == DSRT_OK && v.num_bvh_nodes == 1, "a single leaf");
        pose_all_and_check(hs, "empty body 0");
        hostile(hs);
        EXPECT(dsrt_host_scene_begin_body(hs) == 2, "body 2");
        add(hs, grid(3, 3, 0, 0.5f, 5, 2));
        EXPECT(dsrt_host_scene_build_bvh_bodies(hs) == DSRT_OK, "bodies tree");
        pose_all_and_check(hs, "empty body 0, two movable");
        dsrt_host_scene_destroy(hs);
    }
    {   // 15 movable bodies, some of them empty; the 16th is refused
        DsrtHostScene* hs = dsrt_host_scene_create();
        add(hs, grid(-2, -2, 0, 1, 4, 4));
        for (int b = 1; b < DSRT_MAX_BODIES; ++b) {
            EXPECT(dsrt_host_scene_begin_body(hs) == b, "begin_body");
            if (b % 5 != 0) add(hs, grid(3.0f * (float)b, 0, 1, 0.5f, 1 + b % 4, 1 + b % 3));
        }
        EXPECT(dsrt_host_scene_begin_body(hs) == DSRT_ERR_INVALID, "a 17th body");
        EXPECT(dsrt_host_scene_body_count(hs) == DSRT_MAX_BODIES, "16 bodies");
        EXPECT(dsrt_host_scene_build_bvh_bodies(hs) == DSRT_OK, "bodies tree");
        EXPECT(dsrt_host_scene_bvh_stack_need(hs) >= 11 && dsrt_host_scene_bvh_stack_need(hs) <= 64, "the chain's depth");
        pose_all_and_check(hs, "15 bodies");
        hostile(hs);
        dsrt_host_scene_destroy(hs);
    }
    {   // an empty scene, and null scenes
        DsrtHostScene* hs = dsrt_host_scene_create();
        EXPECT(dsrt_host_scene_build_bvh_bodies(hs) == DSRT_OK, "empty scene");
        EXPECT(dsrt_host_scene_begin_body(hs) == 1, "body 1 of nothing");
        EXPECT(dsrt_host_scene_build_bvh_bodies(hs) == DSRT_OK, "empty bodies");
        const float one[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
        EXPECT(dsrt_host_scene_set_body_poses(hs, 1, 1, one) == DSRT_OK, "posing an empty body");
        hostile(hs);
        dsrt_host_scene_destroy(hs);
        EXPECT(dsrt_host_scene_begin_body(nullptr) == DSRT_ERR_INVALID && dsrt_host_scene_build_bvh_bodies(nullptr) == DSRT_ERR_INVALID, "null scene");
    }
    if (g_failures) { std::fprintf(stderr, "bodies sanitize driver: %d failures\n", g_failures); return 1; }
    std::printf("bodies sanitize driver: ok\n");
    return 0;
}
