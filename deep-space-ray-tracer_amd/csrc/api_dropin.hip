// api_dropin.hip -- the drop-in layer: the reference's own entry points (build_gpu_scene, gpu_render_scene, free_gpu_scene) on one process-wide context with its
// cache of the converted scene.  Calls the public entry points of api_context.hip and api_render.hip and the content-hash launcher of selftest_kernel.hip.
#include <cassert>
#include <cstdlib>
#include <mutex>

#include "api_internal.h"

using namespace dsrt;

// =========================================================================================
// Drop-in layer
// =========================================================================================
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

void gpu_render_scene_body(const GPUScene* scene, int width, int height) {
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
}  // namespace

extern "C" {

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
