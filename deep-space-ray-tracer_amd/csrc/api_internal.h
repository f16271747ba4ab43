// api_internal.h -- what the files of the device half of the C ABI (include/dsrt.h) share: scene_pack.hip and api_*.hip.  Context, scene upload + re-layout,
// render launch, tile de-interleave, and the reference's own entry points on top of them.  Only what two or more of those files use is here; a function that
// crosses files is declared here and nowhere else, and the file that defines it includes this header too.  Not installed; nothing of it is exported.
//
// Replaces: the cudaMalloc/cudaMemcpy half of build_gpu_scene (src/gpu_scene_builder.cpp:322-331, 475-546),
// free_gpu_scene (:603-626) and the host launcher gpu_render_scene (src/gpu_render.cu:1037-1108).
// Differences by design: the scene is converted once into the traversal layout of device_layout.h and stays
// resident across frames (the reference re-uploads everything per frame, src/main.cpp:405); errors are returned,
// not only printed; the launch is asynchronous on a caller-supplied stream; output goes to caller-owned buffers.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/dsrt.h"
#include "../host/host_internal.hpp"
#include "device_layout.h"
#include "hip_check.h"
#include "launchers.h"

#pragma GCC visibility push(hidden)

namespace dsrt {

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
inline FrameState frame_of(const GPUScene& s) { return FrameState{s.camera, s.sun_dir, s.sun_radiance, s.sun_enabled ? 1 : 0}; }

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
    std::vector<int> first_tri, num_tris;          // n_bodies each: the bodies' triangle ranges (dsrt_host_scene_body_range)
    float host_poses[kMaxBodies * 12] = {};        // the poses the resident scene has now (identity after the upload): what a temporal frame with bodies calls `cur`
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

inline float4 as_f4(float a, float b, float c, float d) { return make_float4(a, b, c, d); }

// The 12-float camera block of FrameParams / BatchFrame / GBufferArgs (device_layout.h, kCamOrigin ...).
inline void pack_camera(const GPUCamera& c, float (&cam)[12]) {
    const float cam12[12] = {c.origin.x, c.origin.y, c.origin.z, c.lower_left_corner.x, c.lower_left_corner.y, c.lower_left_corner.z,
                             c.horizontal.x, c.horizontal.y, c.horizontal.z, c.vertical.x, c.vertical.y, c.vertical.z};
    std::memcpy(cam, cam12, sizeof cam12);
}
// The 21-float camera block of TemporalArgs / StarsArgs (launchers.h): those twelve and the basis u, v, w.
inline void pack_camera21(const GPUCamera& c, float (&cam)[21]) {
    static_assert(offsetof(GPUCamera, w) == 18 * sizeof(float), "origin, lower_left_corner, horizontal, vertical, u, v, w: the first 21 floats of GPUCamera");
    std::memcpy(cam, &c, sizeof cam);
}

inline float bits(int i) { float f; std::memcpy(&f, &i, 4); return f; }

// What pack_tree knows about where things went, for a caller that asks (dsrt_scene_upload_bodies): per node record its node and depth, per pair record its one or
// two source triangles (-1 = none).  A leaf's first pair record is in its reference.
struct PackReport { std::vector<int> record_node, record_depth; std::vector<int2> pair_src; };

constexpr size_t kQueueLightWord = 96;                       // the light queue's counter: its own cache line, past the counters
constexpr size_t kCtrlWords = kQueueLightWord + 16;

}  // namespace dsrt

struct DsrtContext {
    int device = 0;
    int num_cus = 0;
    // The resident scene is shared between a context and its clones (dsrt_ctx_clone): one copy in HBM however many frames are in
    // flight.  Camera and sun are per context (they are what changes per frame); so are the working buffers below.
    std::shared_ptr<dsrt::PackedScene> scene;
    dsrt::FrameState frame;
    bool want_second_tree = false;  // dsrt_ctx_set_certified_tree / DSRT_CERTIFIED_TREE: the next upload also builds and packs the certified second tree
    dsrt::DevBuf<uint32_t> ctrl;          // [0] queue, [1] flags, then counters (uint64 x kNumCounters) at byte 16
    dsrt::DevBuf<uint2> spill;
    dsrt::DevBuf<uint32_t> tile_cost, tile_order, tile_work, tile_tmp, probe_queue;
    dsrt::DevBuf<dsrt::BatchFrame> batch_table;  // dsrt_render_batch: one entry per frame
    std::vector<dsrt::BatchFrame> batch_host;
    dsrt::DevBuf<unsigned long long> accum_fixed;
    dsrt::DevBuf<uint32_t> pixel_list;    // dsrt_render_accumulate_masked: the lists of active pixels (one entry per pixel of the shard's tiles)
    dsrt::DevBuf<uint32_t> active_count;  // dsrt_select_unconverged: the word h_active is read from
    dsrt::DevBuf<uint8_t> adaptive_mask;  // dsrt_render_adaptive: the mask between its passes
    dsrt::DevBuf<uint32_t> gb_status;     // dsrt_render_gbuffer's status word
    dsrt::DevBuf<uint32_t> rc_status;     // dsrt_trace_rays' status word
    dsrt::DevBuf<float4> dn_cl[2], dn_vl[2], dn_nr, dn_xf, dn_al;   // dsrt_denoise_accumulated: 7 records of 16 bytes per pixel (launchers.h, DenoiseBuffers)
    dsrt::DevBuf<float4> up_rec[5];       // dsrt_upscale_guided[_coverage]: 5 records of 16 bytes per LOW-resolution pixel (launchers.h, UpscaleRecords)
    dsrt::DevBuf<float> sn_psf;           // dsrt_sensor_apply: the taps on the device, and what they hold now (a call with the same taps uploads nothing)
    std::vector<float> sn_psf_host;
    dsrt::DevBuf<uint32_t> st_list, st_ctrl;          // dsrt_render_stars: the projected stars' indices; {the list's length, the status word}
    dsrt::DevBuf<unsigned long long> st_acc;          // ... and the fixed-point frame the deposits are summed in, width*height*3
    bool st_acc_clean = false;                        // every word of st_acc is zero: the resolve kernel puts back the zeros, so only a new or a doubtful buffer is cleared
    // dsrt_render_denoised_temporal_to_host: the sequence the context keeps -- two histories (tp_hist[tp_cur] holds the last frame's), that frame's camera and size
    dsrt::DevBuf<float4> tp_hist[2];
    GPUCamera tp_camera{};
    float tp_poses[dsrt::kMaxBodies * 12] = {};   // ... and, with tp_bodies, the poses the resident scene's bodies had in that frame
    int tp_cur = 0, tp_width = 0, tp_height = 0;
    bool tp_valid = false;
    bool tp_bodies = false;         // dsrt_ctx_set_temporal_bodies: the sequence follows the bodies instead of ending with a pose update
    int tp_shading = 0;             // dsrt_ctx_set_temporal_shading: 0 off, 1 the sun-state tap test, 2 with the edge guards
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t done = nullptr;      // recorded behind every render: the next render on ANY stream waits for it (queue words, spill strip,
    bool done_valid = false;        // pre-pass arrays and partial sums are per context, so a context has one render in flight)
    ~DsrtContext() { if (ev0) (void)hipEventDestroy(ev0); if (ev1) (void)hipEventDestroy(ev1); if (done) (void)hipEventDestroy(done); }
};

namespace dsrt {

inline float inv_gamma_of(const DsrtRenderDesc& d) { return 1.0f / (d.gamma > 0.0f ? d.gamma : 1.0f); }        // gamma <= 0 is 1, src/gpu_render.cu:1043

uint32_t experiment_word();                        // api_context.hip: the development-switch word

// The context's resident scene, or null ...
inline const PackedScene* scene_of(const DsrtContext* ctx) { return ctx && ctx->scene && ctx->scene->valid ? ctx->scene.get() : nullptr; }
// ... and for an entry point that needs one: null leaves "<fn>: no scene uploaded" as the error, and the caller returns DSRT_ERR_NO_SCENE.
inline const PackedScene* resident_scene(const DsrtContext* ctx, const char* fn) {
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
inline int launch_begin(DsrtContext* ctx, hipStream_t stream, std::initializer_list<Zeroed> zeroed) {
    if (ctx->done_valid) HIP_TRY(hipStreamWaitEvent(stream, ctx->done, 0));
    for (const Zeroed& z : zeroed) if (z.p) HIP_TRY(hipMemsetAsync(z.p, 0, z.bytes, stream));
    return DSRT_OK;
}
inline int launch_clock(DsrtContext* ctx, hipStream_t stream, const DsrtStats* stats) { if (stats) HIP_TRY(hipEventRecord(ctx->ev0, stream)); return DSRT_OK; }
inline int launch_finish(DsrtContext* ctx, hipStream_t stream, DsrtStats* stats) {
    HIP_TRY(hipEventRecord(ctx->done, stream));
    ctx->done_valid = true;
    if (!stats) return DSRT_OK;
    HIP_TRY(hipEventRecord(ctx->ev1, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    std::memset(stats, 0, sizeof *stats);
    HIP_TRY(hipEventElapsedTime(&stats->kernel_ms, ctx->ev0, ctx->ev1));
    return DSRT_OK;
}
inline int flags_result(const char* kernel, uint32_t flags) {
    if (!flags) return DSRT_OK;
    char buf[96];
    std::snprintf(buf, sizeof buf, "%s kernel raised status flags 0x%x", kernel, flags);
    set_error(buf);
    return DSRT_ERR_DEVICE_FLAG;
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

// A struct of pointers and nothing else (include/dsrt.h's, FrameBuffers) from the mirrors of its Staged entries.
template <typename S>
S pointers_as(void* const* mirrors) {              // the caller's list has sizeof(S) / sizeof(void*) entries from `mirrors` on, in S's order
    static_assert(std::is_trivially_copyable_v<S> && sizeof(S) % sizeof(void*) == 0, "a struct of pointers and nothing else");
    S s; std::memcpy(&s, mirrors, sizeof s); return s;
}

inline bool ranges_overlap(const Staged& a, const Staged& b) {
    if (!a.host || !b.host || !a.bytes || !b.bytes) return false;
    const uintptr_t a0 = (uintptr_t)a.host, b0 = (uintptr_t)b.host;
    return a0 < b0 + b.bytes && b0 < a0 + a.bytes;
}

// A SAMPLE-SET FRAME'S BUFFERS, once: the sums and counts, the denoiser's guides, the image outputs and the temporal stage's four, each with its bytes per pixel, its
// direction and the alignment its kernel needs.  check_denoise walks the table; the _to_host forms stage it (staged_frame_call).  A form leaves what it does not take null.
// The upscaler (dsrt_upscale_guided) has two rasters: the rows above are then the OUTPUT resolution's (its guides and images), and its own rows hold what it reads and
// writes at the LOW resolution (`lo` in the table: that raster's pixel count sizes them), the output raster's flags and the support.
struct FrameBuffers {
    const void *sum, *sum_sq, *n;                                      // DsrtAccum, then the per-pixel counts
    const void *normal, *position, *albedo, *range;                    // DsrtDenoiseGuides
    const void *alpha;                                                 // dsrt_denoise_accumulated_coverage's per-pixel coverage
    const void *rgb8, *f32, *linear, *var;                             // the image outputs
    const void *history_prev, *history_next, *prev_xy, *weight;        // the temporal stage's ...
    const void *prim_id, *prev_position;                               // ... and its motion stage's (dsrt_denoise_temporal_bodies)
    const void *shade_flags, *status;                                  // ... and its sun state's (dsrt_denoise_temporal_shaded): the current G-buffer's flags, the status byte
    const void *lo_linear, *lo_var, *lo_normal, *lo_position, *lo_albedo, *lo_range, *lo_flags, *lo_rgb8;      // the upscaler's, low resolution ...
    const void *flags, *support;                                       // ... and output resolution
    const void *lo_alpha, *level;                                      // dsrt_upscale_guided_coverage's: the low-resolution alpha (the output raster's is `alpha` above), the level byte
};
struct FrameBufferKind { size_t bytes; Dir dir; size_t align; bool lo = false; };
constexpr size_t kHistoryBytes = 64;                                   // per pixel: include/dsrt.h, TEMPORAL ACCUMULATION
inline constexpr FrameBufferKind kFrameBuffers[] = {
    {24, Dir::In, 8}, {24, Dir::In, 8}, {4, Dir::In, 4},                                                  // (bytes per pixel, direction, alignment) in FrameBuffers' order,
    {12, Dir::In, 4}, {12, Dir::In, 4}, {12, Dir::In, 4}, {4, Dir::In, 4},                                // a row of this table per row of the struct
    {4, Dir::In, 4},
    {3, Dir::Out, 1}, {12, Dir::Out, 4}, {12, Dir::Out, 4}, {12, Dir::Out, 4},
    {kHistoryBytes, Dir::In, 16}, {kHistoryBytes, Dir::Out, 16}, {8, Dir::Out, 4}, {4, Dir::Out, 4},
    {4, Dir::In, 4}, {12, Dir::Out, 4},
    {1, Dir::In, 1}, {1, Dir::Out, 1},
    {12, Dir::In, 4, true}, {12, Dir::In, 4, true}, {12, Dir::In, 4, true}, {12, Dir::In, 4, true}, {12, Dir::In, 4, true}, {4, Dir::In, 4, true}, {1, Dir::In, 1, true},
    {3, Dir::Out, 1, true}, {1, Dir::In, 1}, {4, Dir::Out, 4},
    {4, Dir::In, 4, true}, {1, Dir::Out, 1}};
constexpr size_t kFrameBufferCount = sizeof(FrameBuffers) / sizeof(void*);
static_assert(sizeof kFrameBuffers / sizeof kFrameBuffers[0] == kFrameBufferCount, "kFrameBuffers has one entry per pointer of FrameBuffers");

inline void frame_table(const FrameBuffers& b, size_t px, Staged (&s)[kFrameBufferCount], size_t px_lo = 0) {
    const void* p[kFrameBufferCount];
    std::memcpy(p, &b, sizeof p);
    for (size_t k = 0; k < kFrameBufferCount; ++k) s[k] = Staged{p[k], (kFrameBuffers[k].lo ? px_lo : px) * kFrameBuffers[k].bytes, kFrameBuffers[k].dir};
}
static_assert(sizeof(DsrtAccum) == 2 * sizeof(void*), "DsrtAccum is {sum, sum_sq}: the first two mirrors of the accumulate and resolve host forms");
inline DsrtAccum accum_of(const FrameBuffers& b) { return DsrtAccum{(uint64_t*)b.sum, (uint64_t*)b.sum_sq}; }

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

// A frame's sums, counts and guides on the device for the length of a _to_host call, sums and counts zeroed, with the views of them the entry points take.
struct FrameScratch {
    DevBuf<unsigned long long> sum, sq;
    DevBuf<uint32_t> n;
    DevBuf<float> normal, position, albedo, range;
    DsrtAccum acc{};
    DsrtDenoiseGuides guides{};
    DevBuf<int32_t> prim_id;
    DevBuf<uint8_t> flags;
    DsrtGBuffer gb{};                                                  // the guides' four channels and, `with_prim_id` / `with_flags`, those
    int init(size_t px, bool counts, bool with_guides, bool with_prim_id = false, bool with_flags = false) {
        int rc;
        if (with_prim_id) { if ((rc = prim_id.alloc(px))) return rc; gb.prim_id = prim_id.p; }
        if (with_flags) { if ((rc = flags.alloc(px))) return rc; gb.flags = flags.p; }
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

// What a batch launch adds to a render: the frames' cameras and sun directions (the context's own camera is not used).
struct BatchInput { int frames; const GPUCamera* cameras; const DsrtF3* sun_dirs; };
// What an accumulate launch changes (dsrt_render_accumulate, checked there): the samples rendered -- {first + j*stride : 0 <= j < count} of a frame
// planned at desc->spp -- and where their sums go (the caller's buffers, added to, never cleared; no resolve).
// mask (dsrt_render_accumulate_masked; null = every pixel): only the pixels whose byte is set; n (optional): their sample counts, `count` added.
struct AccumInput { int first, count, stride; unsigned long long* sum; unsigned long long* sum_sq; const uint8_t* mask; uint32_t* n; };

// ---- The functions that cross files, each defined in the file named ----

// scene_pack.hip
int install_scene(DsrtContext* ctx, const GPUScene& host_layout, const DsrtHostScene* bodies = nullptr);
// api_bodies.hip
int build_bodies(const DsrtHostScene& hs, const PackReport& rep, PackedScene& sc);
// api_render.hip
int render_impl(DsrtContext* ctx, const DsrtRenderDesc* desc, uint8_t* d_rgb8, float* d_f32, void* stream_v, DsrtStats* stats, const BatchInput* batch,
                const AccumInput* acc = nullptr);
// api_sample_sets.hip
int accum_fail(const char* fn, const char* why);
int check_frame_desc(const char* fn, const DsrtRenderDesc* desc, bool renders, bool limit_2_31);
int check_sample_set(const char* fn, const DsrtContext* ctx, const DsrtRenderDesc* desc, int first, int count, int stride);

}  // namespace dsrt

#pragma GCC visibility pop
