// api_context.hip -- the context and its lifetime, the process-wide development-switch word, and the scene uploads that need no more than the packer.
// Calls scene_pack.hip (install_scene); every other file reads the switch word through experiment_word().
#include <atomic>
#include <cassert>
#include <cstdlib>
#include <mutex>

#include "api_internal.h"

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

}  // namespace

uint32_t dsrt::experiment_word() { return g_experiment.load(); }

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

int dsrt_ctx_scene_bounds(const DsrtContext* ctx, float lo[3], float hi[3]) {
    if (!ctx || !lo || !hi) { set_error("dsrt_ctx_scene_bounds: null argument"); return DSRT_ERR_INVALID; }
    const PackedScene* sc = resident_scene(ctx, "dsrt_ctx_scene_bounds");
    if (!sc) return DSRT_ERR_NO_SCENE;
    for (int a = 0; a < 3; ++a) { lo[a] = sc->view.root_lo[a]; hi[a] = sc->view.root_hi[a]; }
    return DSRT_OK;
}

}  // extern "C"
