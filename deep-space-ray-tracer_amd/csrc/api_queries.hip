// api_queries.hip -- what asks the resident scene a question without rendering it: the G-buffer pass, the coverage pass and the batched ray queries, device and
// host forms.  Calls the launchers of gbuffer_kernel.hip, coverage_kernel.hip and raycast_kernel.hip; api_reconstruct.hip's convenience forms call
// dsrt_render_gbuffer and dsrt_render_coverage.
#include <algorithm>
#include <type_traits>

#include "api_internal.h"

using namespace dsrt;

namespace {

// All of it (api_internal.h, ONE LAUNCH AT A TIME PER CONTEXT) around a kernel without a pre-pass and with one status word of its own (the G-buffer pass, the ray queries).
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

// Bytes per element of the channels of include/dsrt.h's structs of pointers, in the order of their members.
constexpr size_t kRayBytes[4] = {12, 12, 4, 4};                                // DsrtRays: origins, dirs, t_min, t_max
constexpr size_t kRayHitBytes[9] = {4, 4, 12, 12, 8, 12, 4, 4, 1};             // DsrtRayHits: t, range, position, normal, uv, albedo, prim_id, material_id, flags
constexpr size_t kGBufferBytes[11] = {4, 4, 4, 12, 12, 8, 12, 4, 4, 4, 1};     // DsrtGBuffer: t, range, depth, position, normal, uv, albedo, prim_id, material_id, sun_cos, flags
static_assert(sizeof(DsrtRays) == 4 * sizeof(void*), "kRayBytes has one entry per pointer of DsrtRays");
static_assert(sizeof(DsrtRayHits) == 9 * sizeof(void*), "kRayHitBytes has one entry per pointer of DsrtRayHits");
static_assert(sizeof(DsrtGBuffer) == 11 * sizeof(void*), "kGBufferBytes has one entry per pointer of DsrtGBuffer");
constexpr int kRayHitFlags = 8;                                               // `flags` in kRayHitBytes: the one channel DSRT_TRACE_ANY writes
static_assert(offsetof(DsrtRayHits, flags) == kRayHitFlags * sizeof(void*) && kRayHitBytes[kRayHitFlags] == 1, "kRayHitFlags is the place of DsrtRayHits.flags");

// Such a struct's channels of `n` elements each as Staged entries, and the struct again from the mirrors of those entries.
template <typename S, size_t N>
void channels(const S& s, const size_t (&bytes_per)[N], size_t n, Dir dir, Staged* out) {
    static_assert(sizeof(S) == N * sizeof(void*), "one table entry per pointer of the struct");
    const void* p[N];
    std::memcpy(p, &s, sizeof p);
    for (size_t k = 0; k < N; ++k) out[k] = Staged{p[k], n * bytes_per[k], dir};
}

// What the G-buffer and the coverage pass take from the context and the resident scene: the scene's view, the camera and its optical axis, the sun, the LDS stack's size.
template <typename Args>
void set_view(Args& a, const DsrtContext* ctx, const PackedScene* sc) {
    a.scene = sc->view;
    const GPUCamera& c = ctx->frame.camera;
    pack_camera(c, a.cam);
    a.neg_w[0] = -c.w.x; a.neg_w[1] = -c.w.y; a.neg_w[2] = -c.w.z;
    a.sun_dir[0] = ctx->frame.sun_dir.x; a.sun_dir[1] = ctx->frame.sun_dir.y; a.sun_dir[2] = ctx->frame.sun_dir.z;
    a.sun_enabled = ctx->frame.sun_enabled;
    a.stack_entries = std::max(1, std::min(64, sc->view.stack_need));       // upload refuses trees that need more than 64
}

// The caller's channel pointers into a kernel's argument block: DsrtGBuffer's eleven, or DsrtRayHits' nine (it has no depth and no sun_cos).
template <typename Args, typename Channels>
void set_channels(Args& a, const Channels& c) {
    a.t = c.t; a.range = c.range; a.position = c.position; a.normal = c.normal; a.uv = c.uv; a.albedo = c.albedo;
    a.prim_id = c.prim_id; a.material_id = c.material_id; a.flags = c.flags;
    if constexpr (std::is_same_v<Channels, DsrtGBuffer>) { a.depth = c.depth; a.sun_cos = c.sun_cos; }
}

// Ray queries (raycast_kernel.hip).  Argument checks shared by the device and the host form: every range is known from `count`.
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

// The coverage pass (coverage_kernel.hip).  DsrtCoverage's 7 + 11 channels: bytes per pixel (class_hits: per class) and the alignment each element needs.
constexpr size_t kCoverageOwn = 7, kCoverageChannels = kCoverageOwn + 11, kCoverageClassHits = 6;
constexpr size_t kCoverageBytes[kCoverageChannels] = {1, 4, 8, 1, 4, 8, 1, 4, 4, 4, 12, 12, 8, 12, 4, 4, 4, 1};     // hits, alpha, mask, sun_*, class_hits, then DsrtGBuffer's
constexpr size_t kCoverageAlign[kCoverageChannels] = {1, 4, 8, 1, 4, 8, 1, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 1};
static_assert(sizeof(DsrtCoverage) == kCoverageChannels * sizeof(void*) && offsetof(DsrtCoverage, rep) == kCoverageOwn * sizeof(void*), "kCoverageBytes has one entry per pointer of DsrtCoverage");
static_assert(offsetof(DsrtCoverage, class_hits) == kCoverageClassHits * sizeof(void*), "kCoverageClassHits is the place of DsrtCoverage.class_hits");

int coverage_samples(const DsrtCoverageDesc& cd) {                                // n, or 0 for what is refused
    if (cd.pattern == DSRT_COVERAGE_GRID) return cd.samples >= 1 && cd.samples <= 8 ? cd.samples * cd.samples : 0;
    if (cd.pattern == DSRT_COVERAGE_DIAGONAL) return cd.samples >= 1 && cd.samples <= 64 ? cd.samples : 0;
    return 0;
}

// Everything dsrt_render_coverage refuses short of the missing scene, device and host form alike; `out` receives the channels as Staged entries.
int check_coverage_args(const char* fn, const DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtCoverageDesc* cd, const DsrtCoverageClasses* classes,
                        const DsrtCoverage* cov, Staged (&out)[kCoverageChannels]) {
    auto fail = [&](const char* why) { set_error(std::string(fn) + ": " + why); return DSRT_ERR_INVALID; };
    if (!ctx || !desc || !cd || !cov) return fail("null argument");
    if (desc->width < 2 || desc->height < 2) return fail("width and height must be at least 2 (the camera divides by W-1 and H-1)");
    if (desc->shard_count > 1) return fail("whole images only (shard_count <= 1)");
    if ((unsigned long long)desc->width * (unsigned long long)desc->height >= (1ull << 31)) return fail("image too large (2^31 pixels)");
    if (!coverage_samples(*cd)) return fail("pattern must be DSRT_COVERAGE_GRID with samples in 1..8 or DSRT_COVERAGE_DIAGONAL with samples in 1..64");
    if (classes) {
        if (classes->count < 0 || classes->count > 16) return fail("classes->count must be between 0 and 16");
        for (int c = 0; c < classes->count; ++c) if (classes->num[c] < 0) return fail("a class has a negative num");
    }
    if (cov->class_hits && (!classes || classes->count == 0)) return fail("class_hits needs classes");
    const void* p[kCoverageChannels];
    std::memcpy(p, cov, sizeof p);
    const size_t px = (size_t)desc->width * desc->height;
    bool any = false;
    for (size_t k = 0; k < kCoverageChannels; ++k) {
        out[k] = Staged{p[k], px * kCoverageBytes[k] * (k == kCoverageClassHits && classes ? (size_t)classes->count : 1), Dir::Out};
        any = any || p[k];
        if ((uintptr_t)p[k] & (kCoverageAlign[k] - 1)) return fail("a pointer is not aligned to its element");
    }
    if (!any) return fail("no output");
    return DSRT_OK;
}

}  // namespace

extern "C" {

void dsrt_coverage_defaults(DsrtCoverageDesc* out) {
    if (!out) return;
    out->pattern = DSRT_COVERAGE_DIAGONAL; out->samples = 64;
}

// The coverage pass (coverage_kernel.hip): dsrt_render_gbuffer's envelope around n rays per pixel, one wave per 64 / n pixels.
int dsrt_render_coverage(DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtCoverageDesc* cd, const DsrtCoverageClasses* classes, const DsrtCoverage* cov,
                         void* stream_v, DsrtStats* stats) {
    return dsrt::guarded("dsrt_render_coverage", [&]() -> int {
    Staged ch[kCoverageChannels];
    if (int rc = check_coverage_args("dsrt_render_coverage", ctx, desc, cd, classes, cov, ch)) return rc;
    const PackedScene* sc = resident_scene(ctx, "dsrt_render_coverage");
    if (!sc) return DSRT_ERR_NO_SCENE;
    HIP_TRY(hipSetDevice(ctx->device));
    CoverageArgs a;
    std::memset(&a, 0, sizeof a);
    set_view(a, ctx, sc);
    a.width = desc->width; a.height = desc->height;
    a.pattern = cd->pattern; a.samples = cd->samples;
    a.n = coverage_samples(*cd);
    a.per_wave = 64 / a.n;
    const DsrtGBuffer& gb = cov->rep;
    a.hits = cov->hits; a.alpha = cov->alpha; a.mask = (unsigned long long*)cov->mask;
    a.sun_hits = cov->sun_hits; a.sun_alpha = cov->sun_alpha; a.sun_mask = (unsigned long long*)cov->sun_mask;
    a.class_hits = cov->class_hits;
    if (classes && cov->class_hits) {
        a.n_classes = classes->count;
        std::memcpy(a.class_first, classes->first, sizeof a.class_first); std::memcpy(a.class_num, classes->num, sizeof a.class_num);
    }
    set_channels(a, gb);
    a.want_sun = cov->sun_hits || cov->sun_alpha || cov->sun_mask || gb.flags;
    for (size_t k = kCoverageOwn; k < kCoverageChannels; ++k) a.want_rep = a.want_rep || ch[k].host;
    if (int rc = ctx->gb_status.grow(1)) return rc;                          // (one launch at a time per context: the G-buffer pass's word serves)
    a.status = ctx->gb_status.p;
    const size_t px = (size_t)desc->width * desc->height;
    const int blocks = (int)((px + (size_t)a.per_wave - 1) / (size_t)a.per_wave);
    return launch_enveloped(ctx, (hipStream_t)stream_v, a.status, stats, "coverage", blocks, [&](hipStream_t s) { return launch_coverage(a, blocks, s); });
    });
}

int dsrt_render_coverage_to_host(DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtCoverageDesc* cd, const DsrtCoverageClasses* classes, const DsrtCoverage* cov,
                                 DsrtStats* stats) {
    return dsrt::guarded("dsrt_render_coverage_to_host", [&]() -> int {
    Staged s[kCoverageChannels];
    if (int rc = check_coverage_args("dsrt_render_coverage_to_host", ctx, desc, cd, classes, cov, s)) return rc;
    if (!resident_scene(ctx, "dsrt_render_coverage_to_host")) return DSRT_ERR_NO_SCENE;
    HIP_TRY(hipSetDevice(ctx->device));
    DsrtStats local;
    return staged_call(s, [&](void* const* d) {
        const DsrtCoverage dc = pointers_as<DsrtCoverage>(d);
        return dsrt_render_coverage(ctx, desc, cd, classes, &dc, nullptr, stats ? stats : &local);
    });
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
    set_view(a, ctx, sc);
    a.width = desc->width; a.height = desc->height;
    a.tiles_x = (desc->width + 7) / 8;
    const int tiles = a.tiles_x * ((desc->height + 7) / 8);
    set_channels(a, *gb);
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
    set_channels(a, *hits);
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

}  // extern "C"
