// api_sample_sets.hip -- sample sets and adaptive sampling: the accumulate, resolve, masked, select and adaptive entry points and what they refuse.
// Calls api_render.hip (render_impl) and the launchers of sample_set_kernel.hip; api_reconstruct.hip shares the checks of a frame's description declared in api_internal.h.
#include "api_internal.h"

using namespace dsrt;

// ---- Sample sets (include/dsrt.h, dsrt_render_accumulate): rng_mode 1 sums of any set of a pixel's samples, added into caller-owned buffers ----
int dsrt::accum_fail(const char* fn, const char* why) { set_error(std::string(fn) + ": " + why); return DSRT_ERR_INVALID; }

// What every entry point over a frame's sums refuses of `desc`, checked like everything below before any HIP call and before anything is written.  Where the
// entry points differ, a parameter says so: a launch that renders (`renders`) words the rng_mode refusal for its caller and leaves math_mode and the size to
// plan_render; the denoiser numbers pixels with 31 bits (`limit_2_31`).  (samples_done: check_sums, check_denoise; collect_counters: check_masked_desc.)
int dsrt::check_frame_desc(const char* fn, const DsrtRenderDesc* desc, bool renders, bool limit_2_31) {
    if (desc->rng_mode != 1) return accum_fail(fn, renders ? "sample sets need rng_mode 1 (rng_mode 0 draws a pixel's samples from one serial stream)" : "accumulated sums are rng_mode 1's");
    if (!renders && desc->math_mode != 0 && desc->math_mode != 1) return accum_fail(fn, "math_mode must be 0 or 1");
    if (desc->shard_count > 1) return accum_fail(fn, "sample sets of tile shards (shard_count > 1) are not supported");
    if (!renders && (desc->width < 2 || desc->height < 2)) return accum_fail(fn, "width and height must be >= 2");
    if (limit_2_31 && (unsigned long long)desc->width * (unsigned long long)desc->height >= (1ull << 31)) return accum_fail(fn, "image too large (2^31 pixels)");
    return DSRT_OK;
}

// Everything dsrt_render_accumulate refuses: of the context, the frame and the set (ctx and desc are given) ...
int dsrt::check_sample_set(const char* fn, const DsrtContext* ctx, const DsrtRenderDesc* desc, int first, int count, int stride) {
    if (!resident_scene(ctx, fn)) return DSRT_ERR_NO_SCENE;
    if (int rc = check_frame_desc(fn, desc, true, false)) return rc;
    if (first < 0) return accum_fail(fn, "first < 0");
    if (count < 1) return accum_fail(fn, "count < 1");
    if (stride < 1) return accum_fail(fn, "stride < 1");
    const long long spp = desc->spp < 1 ? 1 : desc->spp;
    if ((long long)first + (long long)(count - 1) * (long long)stride >= spp) return accum_fail(fn, "the set reaches past the frame's planned samples (first + (count - 1) * stride >= spp)");
    return DSRT_OK;
}

namespace {

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
int accumulate_impl(const char* fn, DsrtContext* ctx, const DsrtRenderDesc* desc, int first, int count, int stride, const DsrtAccum* acc, bool masked, const uint8_t* d_mask,
                    uint32_t* d_n, void* stream, DsrtStats* stats) {
    if (int rc = check_accumulate(fn, ctx, desc, first, count, stride, acc, masked, d_mask)) return rc;
    const AccumInput in{first, count, stride, (unsigned long long*)acc->sum, (unsigned long long*)acc->sum_sq, d_mask, d_n};
    return render_impl(ctx, desc, nullptr, nullptr, stream, stats, nullptr, &in);
}

// ... and their _to_host forms: sums and counts in and out.
struct AccumMirrors { DsrtAccum acc; const uint8_t* mask; uint32_t* n; };        // the staged list below, by name
int accumulate_to_host(const char* fn, DsrtContext* ctx, const DsrtRenderDesc* desc, int first, int count, int stride, const DsrtAccum* h_acc, bool masked, const uint8_t* h_mask,
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
int check_sums(const char* fn, const DsrtContext* ctx, const DsrtRenderDesc* desc, bool have_args, bool have_sum, bool have_sq, const int* samples_done, bool need_sq,
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
int resolve_sums(const char* fn, DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtAccum* acc, bool per_pixel, int samples_done, const uint32_t* d_n, uint8_t* d_rgb8,
                 float* d_f32, float* d_var_of_mean, hipStream_t stream) {
    const void* outputs[3] = {d_rgb8, d_f32, d_var_of_mean};
    int rc = check_sums(fn, ctx, desc, acc && (d_n || !per_pixel), acc && acc->sum, acc && acc->sum_sq, per_pixel ? nullptr : &samples_done, d_var_of_mean != nullptr, outputs);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    if ((rc = launch_begin(ctx, stream, {}))) return rc;                             // the context's last launch (an accumulate into these sums, maybe) comes first
    const bool device_libm = desc->math_mode == 1;
    const size_t px = (size_t)desc->width * desc->height;
    const unsigned long long* sum = (const unsigned long long*)acc->sum;
    const unsigned long long* sq = d_var_of_mean ? (const unsigned long long*)acc->sum_sq : nullptr;       // (the second moment serves the variance only)
    HIP_TRY(per_pixel ? launch_resolve_counts(sum, d_n, inv_gamma_of(*desc), device_libm, px, d_rgb8, d_f32, sq, d_var_of_mean, stream)
                      : launch_resolve(sum, samples_done, inv_gamma_of(*desc), device_libm, px, d_rgb8, d_f32, sq, d_var_of_mean, stream));
    return DSRT_OK;
}

// ---- Adaptive sampling (include/dsrt.h, ADAPTIVE SAMPLING): masked sample sets, the convergence test that makes the masks, the per-pixel resolve, the driver ----
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

extern "C" {

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

}  // extern "C"
