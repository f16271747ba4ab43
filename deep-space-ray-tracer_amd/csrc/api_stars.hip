// api_stars.hip -- the star field's entry points (include/dsrt.h, POINT SOURCES): dsrt_render_stars and its _to_host form.  Calls the launcher of stars_kernel.hip.
// The catalogue helpers need no device and live in host/stars_host.cpp.
#include <algorithm>

#include "api_internal.h"

using namespace dsrt;

namespace {

constexpr int kMaxStars = 1 << 22;

// The call's seven buffers, device or host form alike: the three inputs, then the four outputs as the caller gave them (one not asked for is null).
struct StarBuffers { Staged s[7]; };
StarBuffers star_buffers(size_t px, size_t count, const DsrtStars* in, const DsrtStarsOut* out) {
    return StarBuffers{{{in->dir, count * 3 * sizeof(float), Dir::In}, {in->flux, count * 3 * sizeof(float), Dir::In}, {in->linear_in, px * 3 * sizeof(float), Dir::In},
                        {out->layer, px * 3 * sizeof(float), Dir::Out}, {out->linear_out, px * 3 * sizeof(float), Dir::Out}, {out->xy, count * 2 * sizeof(float), Dir::Out},
                        {out->status, count, Dir::Out}}};
}

// Everything dsrt_render_stars refuses short of the missing scene, before anything is launched or written; the same for the host form's host pointers.
int check_stars(const char* fn, const DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtStars* in, const DsrtStarsOut* out) {
    if (!ctx || !desc || !in || !out) return accum_fail(fn, "null argument");
    if (desc->width < 2 || desc->height < 2) return accum_fail(fn, "width and height must be >= 2");
    if ((unsigned long long)desc->width * (unsigned long long)desc->height >= (1ull << 31)) return accum_fail(fn, "image too large (2^31 pixels)");
    if (in->count < 0 || in->count > kMaxStars) return accum_fail(fn, "count must be between 0 and 2^22");
    if (in->count > 0 && (!in->dir || !in->flux)) return accum_fail(fn, "null dir or flux with count > 0");
    if (!out->layer && !out->linear_out && !out->xy && !out->status) return accum_fail(fn, "no output");
    if (out->linear_out && !in->linear_in) return accum_fail(fn, "linear_out needs linear_in");
    const StarBuffers b = star_buffers((size_t)desc->width * (size_t)desc->height, (size_t)in->count, in, out);
    for (int k = 0; k < 6; ++k) if ((uintptr_t)b.s[k].host & 3u) return accum_fail(fn, "pointer not 4-byte aligned");
    for (int o = 3; o < 7; ++o) {
        for (int i = 0; i < 3; ++i) if (ranges_overlap(b.s[o], b.s[i])) return accum_fail(fn, "an output range overlaps an input range");
        for (int q = o + 1; q < 7; ++q) if (ranges_overlap(b.s[o], b.s[q])) return accum_fail(fn, "two output ranges overlap");
    }
    return DSRT_OK;
}

int stars_impl(const char* fn, DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtStars* in, const DsrtStarsOut* out, hipStream_t stream, DsrtStats* stats) {
    int rc;
    if ((rc = check_stars(fn, ctx, desc, in, out))) return rc;
    const PackedScene* sc = resident_scene(ctx, fn);
    if (!sc) return DSRT_ERR_NO_SCENE;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t floats = (size_t)desc->width * (size_t)desc->height * 3;
    const bool image = out->layer || out->linear_out;
    if (image && ctx->st_acc.n < floats) ctx->st_acc_clean = false;         // (a grown buffer's contents are not kept)
    if ((rc = ctx->st_ctrl.grow(2)) || (rc = ctx->st_list.grow((size_t)std::max(in->count, 1))) || (image && (rc = ctx->st_acc.grow(floats)))) return rc;
    StarsArgs a;
    std::memset(&a, 0, sizeof a);
    a.scene = sc->view;
    a.dir = in->dir; a.flux = in->flux; a.linear_in = out->linear_out ? in->linear_in : nullptr;
    a.count = in->count; a.width = desc->width; a.height = desc->height; a.occlusion = in->occlusion != 0;
    a.stack_entries = std::max(1, std::min(64, sc->view.stack_need));       // upload refuses trees that need more than 64
    pack_camera21(ctx->frame.camera, a.cam);
    a.list = ctx->st_list.p; a.list_len = ctx->st_ctrl.p; a.status = ctx->st_ctrl.p + 1;
    a.acc = image ? ctx->st_acc.p : nullptr;
    a.layer = out->layer; a.linear_out = out->linear_out; a.xy = out->xy; a.star_status = out->status;
    // The accumulator is all zeros between calls: the resolve kernel writes back a zero wherever it read a sum.  It is cleared here only when that is not known -- a
    // new allocation, or a call before this one that did not get as far as its resolve launch.
    const bool clear = image && !ctx->st_acc_clean;
    if ((rc = launch_begin(ctx, stream, {{ctx->st_ctrl.p, 2 * sizeof(uint32_t)}, {clear ? (void*)ctx->st_acc.p : nullptr, ctx->st_acc.n * sizeof(unsigned long long)}})) ||
        (rc = launch_clock(ctx, stream, stats))) return rc;
    if (image) ctx->st_acc_clean = false;
    HIP_TRY(launch_stars(a, stream));
    if (image) ctx->st_acc_clean = true;
    if ((rc = launch_finish(ctx, stream, stats)) || !stats) return rc;
    HIP_TRY(hipMemcpy(&stats->device_flags, a.status, sizeof(uint32_t), hipMemcpyDeviceToHost));
    stats->waves_launched = (in->count + 63) / 64;
    return flags_result("star field", stats->device_flags);
}

}  // namespace

extern "C" {

int dsrt_render_stars(DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtStars* stars, const DsrtStarsOut* out, void* stream_v, DsrtStats* stats) {
    return dsrt::guarded("dsrt_render_stars", [&]() -> int { return stars_impl("dsrt_render_stars", ctx, desc, stars, out, (hipStream_t)stream_v, stats); });
}

int dsrt_render_stars_to_host(DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtStars* stars, const DsrtStarsOut* out, DsrtStats* stats) {
    return dsrt::guarded("dsrt_render_stars_to_host", [&]() -> int {
    const char* fn = "dsrt_render_stars_to_host";
    if (int rc = check_stars(fn, ctx, desc, stars, out)) return rc;
    if (!resident_scene(ctx, fn)) return DSRT_ERR_NO_SCENE;
    if (stars->count == 0 && !out->layer && !out->linear_out) {             // per-star outputs of no stars: nothing to stage, nothing to write
        if (stats) std::memset(stats, 0, sizeof *stats);
        return DSRT_OK;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    const StarBuffers h =star_buffers((size_t)desc->width * (size_t)desc->height, (size_t)stars->count, stars, out);
    DsrtStats local;
    return staged_call(h.s, [&](void* const* m) -> int {
        DsrtStars ds = *stars;
        ds.dir = (const float*)m[0]; ds.flux = (const float*)m[1]; ds.linear_in = (const float*)m[2];
        const DsrtStarsOut dout = pointers_as<DsrtStarsOut>(m + 3);
        return stars_impl(fn, ctx, desc, &ds, &dout, nullptr, stats ? stats : &local);
    });
    });
}

}  // extern "C"
