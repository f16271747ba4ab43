// api_reconstruct.hip -- what turns a sample-set frame into an image: the denoiser, its temporal stage and the upscaler, with their _to_host and convenience forms.
// Calls the launchers of denoise_kernel.hip, temporal_kernel.hip and upscale_kernel.hip, the checks of api_sample_sets.hip, and, in the convenience forms, the entry
// points of api_sample_sets.hip (dsrt_render_accumulate) and api_queries.hip (dsrt_render_gbuffer, dsrt_render_coverage).
#include "api_internal.h"

using namespace dsrt;

namespace {

constexpr size_t kFrameTemporal = offsetof(FrameBuffers, history_prev) / sizeof(void*);
constexpr size_t kFrameUpscale = offsetof(FrameBuffers, lo_linear) / sizeof(void*);
constexpr float kUpscaleCoverageAlphaMin = 0.125f;                                    // dsrt_upscale_coverage_alpha_min: likewise (the subsection on the upscaler with coverage)
constexpr float kCoverageAlphaMin = 0.0625f;                                          // dsrt_denoise_coverage_alpha_min: DESIGN.md section 4 says how it was chosen

// The table's entries [from, to) against those before them and among themselves: alignment; then each of their outputs against every input up to `to` (over_input) and
// against every other output not checked against it yet (over_output); then the outputs before `from` against their inputs (old_over_input; nothing to do for from = 0).
int check_frame_table(const char* fn, const Staged (&s)[kFrameBufferCount], size_t from, size_t to, const char* over_input, const char* over_output, const char* old_over_input) {
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

// ---- The denoiser (include/dsrt.h, DENOISER; denoise_kernel.hip): prepare, one a-trous launch per iteration, output.  It reads the caller's sums, counts and guides
// and writes the caller's outputs and the context's own seven records per pixel; the render buffers, camera and sun are not touched.
// Temporal accumulation (include/dsrt.h, TEMPORAL ACCUMULATION; temporal_kernel.hip) is the denoiser with the history stage in front of its iterations. ----

// The temporal stage's part of a call (dsrt_denoise_temporal): null for the plain denoiser.
// `bodies`: the call is dsrt_denoise_temporal_bodies, with its motion (required then; prim_id where the form has its buffers) and its optional X' output.
struct TemporalInput {
    const GPUCamera* prev_camera; const float* prev; float* next; const DsrtTemporal* tp; float* prev_xy; float* weight;
    bool bodies = false; const DsrtBodyMotion* motion = nullptr; float* prev_position = nullptr;
    // `shaded`: the call is dsrt_denoise_temporal_shaded, with its shading (required then; flags where the form has its buffers), its optional status output, and
    // a motion that may be null (`bodies` says whether it is given)
    bool shaded = false; const DsrtTemporalShading* shading = nullptr; uint8_t* status = nullptr;
};

// The coverage part of a call (dsrt_denoise_accumulated_coverage; include/dsrt.h, COVERAGE DEMODULATION): null for the other forms.  A null alpha is the plain denoiser.
struct CoverageInput { const float* alpha; float alpha_min; };

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
FrameBuffers denoise_buffers(const DsrtAccum& acc, const uint32_t* n, const DsrtDenoiseGuides& g, const TemporalInput* t, const void* rgb8, const void* f32, const void* linear, const void* var,
                             const float* alpha = nullptr) {
    return FrameBuffers{acc.sum, acc.sum_sq, n, g.normal, g.position, g.albedo, g.range, alpha, rgb8, f32, linear, var,
                        t ? t->prev : nullptr, t ? t->next : nullptr, t ? t->prev_xy : nullptr, t ? t->weight : nullptr,
                        t && t->motion ? t->motion->prim_id : nullptr, t ? t->prev_position : nullptr,
                        t && t->shading ? t->shading->flags : nullptr, t ? t->status : nullptr};
}

// Everything dsrt_denoise_accumulated and (with `t`) dsrt_denoise_temporal refuse, before anything is launched or written; the same for the host forms' host pointers.
int check_denoise(const char* fn, const DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtAccum* acc, int samples_done, const uint32_t* n, const DsrtDenoiseGuides* guides,
                  const TemporalInput* t, const DsrtDenoise* dn, const uint8_t* rgb8, const float* f32, const float* linear, const float* var, const CoverageInput* cv = nullptr) {
    if (!ctx || !desc || !acc || !guides || !dn) return accum_fail(fn, "null argument");
    if (cv && !(cv->alpha_min > 0.0f && cv->alpha_min <= 1.0f)) return accum_fail(fn, "alpha_min must be > 0 and <= 1");
    if (t && t->bodies) if (int rc = check_body_motion(fn, t->motion)) return rc;
    if (t && t->shaded) {
        if (!t->shading || !t->shading->flags) return accum_fail(fn, "null argument (DsrtTemporalShading or its flags)");
        if (t->shading->edge_guard != 0 && t->shading->edge_guard != 1) return accum_fail(fn, "edge_guard must be 0 or 1");
        if (t->prev_position && !t->motion) return accum_fail(fn, "prev_position needs a motion");
    }
    if (!acc->sum || !acc->sum_sq) return accum_fail(fn, "DsrtAccum.sum or sum_sq is NULL (the filter is guided by the variance: both are required)");
    if (!guides->normal || !guides->position || !guides->albedo || !guides->range) return accum_fail(fn, "a guide channel is NULL (normal, position, albedo and range are required)");
    if (int rc = check_frame_desc(fn, desc, false, true)) return rc;
    if (!n && samples_done < 2) return accum_fail(fn, "samples_done < 2 (the variance needs two samples; pass per-pixel counts otherwise)");
    if (int rc = check_denoise_params(fn, dn)) return rc;
    if (!rgb8 && !f32 && !linear && !var) return accum_fail(fn, "no output");
    Staged s[kFrameBufferCount];
    frame_table(denoise_buffers(*acc, n, *guides, t, rgb8, f32, linear, var, cv ? cv->alpha : nullptr), (size_t)desc->width * desc->height, s);
    if (int rc = check_frame_table(fn, s, 0, kFrameTemporal, "an output range overlaps an input range", "two output ranges overlap", nullptr)) return rc;
    if (!t) return DSRT_OK;
    if ((t->prev_camera != nullptr) != (t->prev != nullptr)) return accum_fail(fn, "the previous camera and the previous history go together: both NULL (first frame) or both given");
    if (!t->next) return accum_fail(fn, "the next history is NULL (it is required)");
    if (int rc = check_temporal_params(fn, t->tp)) return rc;
    return check_frame_table(fn, s, kFrameTemporal, kFrameUpscale, "the next history, prev_xy, weight, prev_position or status overlaps an input or the previous history",
                             "the next history, prev_xy, weight, prev_position or status overlaps another output",
                             "an output range overlaps the previous history, prim_id or flags");
}

// dsrt_denoise_accumulated and dsrt_denoise_temporal: the checks, then prepare, the temporal stage if there is one, the iterations, output.
int denoise_impl(const char* fn, DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtAccum* acc, int samples_done, const uint32_t* d_n, const DsrtDenoiseGuides* guides,
                 const TemporalInput* t, const DsrtDenoise* dn, uint8_t* d_rgb8, float* d_f32, float* d_linear, float* d_var, hipStream_t stream, const CoverageInput* cv = nullptr) {
    int rc;
    if ((rc = check_denoise(fn, ctx, desc, acc, samples_done, d_n, guides, t, dn, d_rgb8, d_f32, d_linear, d_var, cv))) return rc;
    const float* alpha = cv ? cv->alpha : nullptr;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t px = (size_t)desc->width * desc->height;
    // (growing frees the old records: the launch that may still read them has to be over first)
    if (ctx->dn_al.n < px && ctx->done_valid) HIP_TRY(hipEventSynchronize(ctx->done));
    for (int k = 0; k < 2; ++k) if ((rc = ctx->dn_cl[k].grow(px)) || (rc = ctx->dn_vl[k].grow(px))) return rc;
    if ((rc = ctx->dn_nr.grow(px)) || (rc = ctx->dn_xf.grow(px)) || (rc = ctx->dn_al.grow(px))) return rc;
    const DenoiseBuffers b{{ctx->dn_cl[0].p, ctx->dn_cl[1].p}, {ctx->dn_vl[0].p, ctx->dn_vl[1].p}, ctx->dn_nr.p, ctx->dn_xf.p, ctx->dn_al.p};
    if ((rc = launch_begin(ctx, stream, {}))) return rc;                             // the context's last launch (an accumulate into these sums, the G-buffer) comes first
    if (alpha) HIP_TRY(launch_denoise_prepare_coverage((const unsigned long long*)acc->sum, (const unsigned long long*)acc->sum_sq, samples_done, d_n, guides->normal,
                                                       guides->position, guides->albedo, guides->range, alpha, cv->alpha_min, px, b, stream));
    else HIP_TRY(launch_denoise_prepare((const unsigned long long*)acc->sum, (const unsigned long long*)acc->sum_sq, samples_done, d_n, guides->normal, guides->position,
                                        guides->albedo, guides->range, px, b, stream));
    if (t) {
        TemporalArgs a;
        std::memset(&a, 0, sizeof a);
        a.cl = b.cl[0]; a.vl = b.vl[0]; a.nr = b.nr; a.xf = b.xf;
        a.prev = (const float4*)t->prev; a.next = (float4*)t->next; a.prev_xy = t->prev_xy; a.weight = t->weight;
        a.counts = d_n; a.samples_done = samples_done; a.width = desc->width; a.height = desc->height;
        if (t->prev_camera) pack_camera21(*t->prev_camera, a.cam);
        a.alpha_min = t->tp->alpha_min; a.normal_cos_min = t->tp->normal_cos_min; a.plane_tol = t->tp->plane_tol; a.min_support = t->tp->min_support;
        BodyMotionArgs mo;                                                            // (all zero without a motion: no prim_id, no body moved)
        std::memset(&mo, 0, sizeof mo);
        if (t->bodies) {
            BodyMotionTable tab;                                                      // (the motion's host arrays are read here, before the call returns)
            pack_body_motion(*t->motion, tab);
            mo.prim_id = t->motion->prim_id; mo.prev_position = t->prev_position; mo.moved = tab.moved;
            static_assert(sizeof mo.first == sizeof tab.first && sizeof mo.count == sizeof tab.count && sizeof mo.poses == sizeof tab.poses, "BodyMotionArgs carries BodyMotionTable");
            std::memcpy(mo.first, tab.first, sizeof mo.first); std::memcpy(mo.count, tab.count, sizeof mo.count); std::memcpy(mo.poses, tab.poses, sizeof mo.poses);
        }
        ShadingArgs sh{};
        if (t->shaded) sh = ShadingArgs{t->shading->flags, t->status, t->shading->edge_guard};
        // (the stage that follows shading takes the motion stage's argument with or without a motion)
        HIP_TRY(launch_temporal(a, t->bodies || t->shaded ? &mo : nullptr, t->shaded ? &sh : nullptr, stream));
    }
    for (int i = 0; i < dn->iterations; ++i)
        HIP_TRY(launch_denoise_atrous(b, i & 1, desc->width, desc->height, 1 << i, dn->normal_power_log2, dn->sigma_l, dn->sigma_z, dn->sigma_a, stream));
    if (alpha) HIP_TRY(launch_denoise_output_coverage(b, dn->iterations & 1, alpha, px, inv_gamma_of(*desc), desc->math_mode == 1, d_rgb8, d_f32, d_linear, d_var, stream));
    else HIP_TRY(launch_denoise_output(b, dn->iterations & 1, px, inv_gamma_of(*desc), desc->math_mode == 1, d_rgb8, d_f32, d_linear, d_var, stream));
    return launch_finish(ctx, stream, nullptr);                                      // the records are the context's: its next launch on any stream comes behind
}

// Their _to_host forms: the same call on device mirrors of the frame's table, the device finished before the results are copied out.
int denoise_to_host(const char* fn, DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtAccum* h_acc, int samples_done, const uint32_t* h_n, const DsrtDenoiseGuides* h_guides,
                    const TemporalInput* ht, const DsrtDenoise* dn, uint8_t* h_rgb8, float* h_f32, float* h_linear, float* h_var, const CoverageInput* hcv = nullptr) {
    if (int rc = check_denoise(fn, ctx, desc, h_acc, samples_done, h_n, h_guides, ht, dn, h_rgb8, h_f32, h_linear, h_var, hcv)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    const FrameBuffers h = denoise_buffers(*h_acc, h_n, *h_guides, ht, h_rgb8, h_f32, h_linear, h_var, hcv ? hcv->alpha : nullptr);
    return staged_frame_call(h, (size_t)desc->width * desc->height, true, [&](const FrameBuffers& m) {
        const DsrtAccum acc = accum_of(m);
        const DsrtDenoiseGuides g{(const float*)m.normal, (const float*)m.position, (const float*)m.albedo, (const float*)m.range};
        DsrtBodyMotion motion{};                                                      // the caller's, with prim_id's mirror
        if (ht && ht->bodies) { motion = *ht->motion; motion.prim_id = (const int32_t*)m.prim_id; }
        DsrtTemporalShading shading{};                                                // ... and with flags' mirror
        if (ht && ht->shaded) { shading = *ht->shading; shading.flags = (const uint8_t*)m.shade_flags; }
        const TemporalInput t{ht ? ht->prev_camera : nullptr, (const float*)m.history_prev, (float*)m.history_next, ht ? ht->tp : nullptr, (float*)m.prev_xy, (float*)m.weight,
                              ht && ht->bodies, ht && ht->bodies ? &motion : nullptr, (float*)m.prev_position,
                              ht && ht->shaded, ht && ht->shaded ? &shading : nullptr, (uint8_t*)m.status};
        const CoverageInput cv{(const float*)m.alpha, hcv ? hcv->alpha_min : 1.0f};
        return denoise_impl(fn, ctx, desc, &acc, samples_done, (const uint32_t*)m.n, &g, ht ? &t : nullptr, dn, (uint8_t*)m.rgb8, (float*)m.f32, (float*)m.linear,
                            (float*)m.var, nullptr, hcv ? &cv : nullptr);
    });
}

// The convenience forms (dsrt_render_denoised_to_host, and `temporal` dsrt_render_denoised_temporal_to_host): what they refuse; *spp is the frame's samples.
int check_render_denoised(const char* fn, const DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtDenoise* dn, bool temporal, const DsrtTemporal* tp, bool any_output, int* spp) {
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
int render_denoised_to_host(DsrtContext* ctx, const DsrtRenderDesc* desc, int spp, const FrameScratch& f, const TemporalInput* t, const DsrtDenoise* dn, uint8_t* h_rgb8,
                            float* h_f32, float* h_linear, float* h_var, float* h_prev_xy, DsrtStats* stats) {
    FrameBuffers h{};
    h.rgb8 = h_rgb8; h.f32 = h_f32; h.linear = h_linear; h.var = h_var; h.prev_xy = h_prev_xy;
    DsrtStats local;
    return staged_frame_call(h, (size_t)desc->width * (size_t)desc->height, true, [&](const FrameBuffers& m) -> int {
        int r;
        if ((r = dsrt_render_accumulate(ctx, desc, 0, spp, 1, &f.acc, nullptr, stats ? stats : &local))) return r;
        if ((r = dsrt_render_gbuffer(ctx, desc, &f.gb, nullptr, nullptr))) return r;
        if (t && t->shaded)
            return dsrt_denoise_temporal_shaded(ctx, desc, &f.acc, spp, nullptr, &f.guides, t->motion, t->shading, t->prev_camera, t->prev, t->next, t->tp, dn, (uint8_t*)m.rgb8,
                                                (float*)m.f32, (float*)m.linear, (float*)m.var, (float*)m.prev_xy, nullptr, nullptr, nullptr, nullptr);
        if (t && t->bodies)
            return dsrt_denoise_temporal_bodies(ctx, desc, &f.acc, spp, nullptr, &f.guides, t->motion, t->prev_camera, t->prev, t->next, t->tp, dn, (uint8_t*)m.rgb8,
                                                (float*)m.f32, (float*)m.linear, (float*)m.var, (float*)m.prev_xy, nullptr, nullptr, nullptr);
        return t ? dsrt_denoise_temporal(ctx, desc, &f.acc, spp, nullptr, &f.guides, t->prev_camera, t->prev, t->next, t->tp, dn, (uint8_t*)m.rgb8, (float*)m.f32,
                                         (float*)m.linear, (float*)m.var, (float*)m.prev_xy, nullptr, nullptr)
                 : dsrt_denoise_accumulated(ctx, desc, &f.acc, spp, nullptr, &f.guides, dn, (uint8_t*)m.rgb8, (float*)m.f32, (float*)m.linear, (float*)m.var, nullptr);
    });
}

// ---- The upscaler (include/dsrt.h, UPSCALER; upscale_kernel.hip): pack the low-resolution frame, one launch over the output pixels.  It reads the caller's colour,
// variance and the two rasters' guides and writes the caller's outputs and the context's own five records per low-resolution pixel. ----
int check_upscale_params(const char* fn, const DsrtUpscale* up) {
    if (!up) return accum_fail(fn, "null argument (DsrtUpscale)");
    if (up->normal_power_log2 < 0 || up->normal_power_log2 > 8) return accum_fail(fn, "normal_power_log2 must be between 0 and 8");
    if (!(up->sigma_z > 0.0f) || !(up->sigma_a > 0.0f)) return accum_fail(fn, "sigma_z and sigma_a must be > 0");
    return DSRT_OK;
}

// The buffers of an upscaler call, device or host form alike: the shared rows are the output raster's.
// The coverage part of an upscaler call (dsrt_upscale_guided_coverage; include/dsrt.h, COVERAGE-AWARE UPSCALER): null for dsrt_upscale_guided.  Both alphas null is
// the plain upscaler (alpha_min is then only checked).
struct UpscaleCoverageInput { const float* lo_alpha; const float* hi_alpha; float alpha_min; uint8_t* level; };

FrameBuffers upscale_buffers(const float* lo_linear, const float* lo_var, const DsrtUpscaleGuides& lo, const DsrtUpscaleGuides& hi, const void* rgb8, const void* f32,
                             const void* linear, const void* var, const void* support, const UpscaleCoverageInput* cv = nullptr) {
    FrameBuffers b{};
    if (cv) { b.alpha = cv->hi_alpha; b.lo_alpha = cv->lo_alpha; b.level = cv->level; }
    b.normal = hi.normal; b.position = hi.position; b.albedo = hi.albedo; b.range = hi.range; b.flags = hi.flags;
    b.rgb8 = rgb8; b.f32 = f32; b.linear = linear; b.var = var; b.support = support;
    b.lo_linear = lo_linear; b.lo_var = lo_var;
    b.lo_normal = lo.normal; b.lo_position = lo.position; b.lo_albedo = lo.albedo; b.lo_range = lo.range; b.lo_flags = lo.flags;
    return b;
}
DsrtUpscaleGuides lo_guides_of(const FrameBuffers& m) { return DsrtUpscaleGuides{(const float*)m.lo_normal, (const float*)m.lo_position, (const float*)m.lo_albedo, (const float*)m.lo_range, (const uint8_t*)m.lo_flags}; }
DsrtUpscaleGuides hi_guides_of(const FrameBuffers& m) { return DsrtUpscaleGuides{(const float*)m.normal, (const float*)m.position, (const float*)m.albedo, (const float*)m.range, (const uint8_t*)m.flags}; }

// What of the two rasters' sizes is refused (desc's own is check_frame_desc's).
int check_upscale_sizes(const char* fn, int lo_width, int lo_height, int width, int height) {
    if (lo_width < 2 || lo_height < 2) return accum_fail(fn, "lo_width and lo_height must be >= 2");
    if (width < lo_width || height < lo_height) return accum_fail(fn, "the output must be at least as large as the low-resolution frame (W >= lo_width, H >= lo_height)");
    return DSRT_OK;
}

// Everything dsrt_upscale_guided refuses, before anything is launched or written; the same for the host form's host pointers.
int check_upscale(const char* fn, const DsrtContext* ctx, const DsrtRenderDesc* desc, int lo_width, int lo_height, const float* lo_linear, const float* lo_var,
                  const DsrtUpscaleGuides* lo, const DsrtUpscaleGuides* hi, const DsrtUpscale* up, const uint8_t* rgb8, const float* f32, const float* linear,
                  const float* var, const float* support, const UpscaleCoverageInput* cv = nullptr) {
    if (!ctx || !desc || !lo_linear || !lo || !hi || !up) return accum_fail(fn, "null argument");
    for (const DsrtUpscaleGuides* g : {lo, hi})
        if (!g->normal || !g->position || !g->albedo || !g->range) return accum_fail(fn, "a guide channel is NULL (normal, position, albedo and range are required; flags is the optional one)");
    if (int rc = check_frame_desc(fn, desc, false, true)) return rc;
    if (int rc = check_upscale_sizes(fn, lo_width, lo_height, desc->width, desc->height)) return rc;
    if (int rc = check_upscale_params(fn, up)) return rc;
    if (cv) {
        if ((cv->lo_alpha != nullptr) != (cv->hi_alpha != nullptr)) return accum_fail(fn, "the two alphas go together: both NULL (the plain upscaler) or both given");
        if (!(cv->alpha_min > 0.0f && cv->alpha_min <= 1.0f)) return accum_fail(fn, "alpha_min must be > 0 and <= 1");
        if (cv->level && !cv->lo_alpha) return accum_fail(fn, "the level output needs the alphas");
    }
    if (!rgb8 && !f32 && !linear && !var && !support && !(cv && cv->level)) return accum_fail(fn, "no output");
    if (var && !lo_var) return accum_fail(fn, "the variance output needs the low-resolution variance (d_lo_var)");
    Staged s[kFrameBufferCount];
    frame_table(upscale_buffers(lo_linear, lo_var, *lo, *hi, rgb8, f32, linear, var, support, cv), (size_t)desc->width * desc->height, s, (size_t)lo_width * lo_height);
    return check_frame_table(fn, s, 0, kFrameBufferCount, "an output range overlaps an input range", "two output ranges overlap", nullptr);
}

int upscale_impl(const char* fn, DsrtContext* ctx, const DsrtRenderDesc* desc, int lo_width, int lo_height, const float* d_lo_linear, const float* d_lo_var,
                 const DsrtUpscaleGuides* lo, const DsrtUpscaleGuides* hi, const DsrtUpscale* up, uint8_t* d_rgb8, float* d_f32, float* d_linear, float* d_var,
                 float* d_support, hipStream_t stream, const UpscaleCoverageInput* cv = nullptr) {
    int rc;
    if ((rc = check_upscale(fn, ctx, desc, lo_width, lo_height, d_lo_linear, d_lo_var, lo, hi, up, d_rgb8, d_f32, d_linear, d_var, d_support, cv))) return rc;
    const bool coverage = cv && cv->lo_alpha;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t px_lo = (size_t)lo_width * lo_height;
    // (growing frees the old records: the launch that may still read them has to be over first)
    if (ctx->up_rec[4].n < px_lo && ctx->done_valid) HIP_TRY(hipEventSynchronize(ctx->done));
    for (DevBuf<float4>& r : ctx->up_rec) if ((rc = r.grow(px_lo))) return rc;
    const UpscaleRecords rec{ctx->up_rec[0].p, ctx->up_rec[1].p, ctx->up_rec[2].p, ctx->up_rec[3].p, ctx->up_rec[4].p};
    if ((rc = launch_begin(ctx, stream, {}))) return rc;                             // the context's last launch (the denoiser, a G-buffer) comes first
    if (coverage) HIP_TRY(launch_upscale_pack_coverage(d_lo_linear, d_lo_var, lo->normal, lo->position, lo->albedo, lo->range, lo->flags, cv->lo_alpha, px_lo, rec, stream));
    else HIP_TRY(launch_upscale_pack(d_lo_linear, d_lo_var, lo->normal, lo->position, lo->albedo, lo->range, lo->flags, px_lo, rec, stream));
    UpscaleArgs a;
    std::memset(&a, 0, sizeof a);
    a.cr = rec.cr; a.vf = rec.vf; a.nn = rec.nn; a.xx = rec.xx; a.aa = rec.aa;
    a.hi_normal = hi->normal; a.hi_position = hi->position; a.hi_albedo = hi->albedo; a.hi_range = hi->range; a.hi_flags = hi->flags;
    a.out_rgb8 = d_rgb8; a.out_f32 = d_f32; a.out_linear = d_linear; a.out_var = d_var; a.out_support = d_support;
    a.w = lo_width; a.h = lo_height; a.W = desc->width; a.H = desc->height;
    a.normal_power_log2 = up->normal_power_log2; a.use_sun = up->use_sun != 0; a.lo_has_flags = lo->flags != nullptr;
    a.sigma_z = up->sigma_z; a.sigma_a = up->sigma_a; a.inv_gamma = inv_gamma_of(*desc);
    if (coverage) HIP_TRY(launch_upscale_coverage(UpscaleCoverageArgs{a, cv->hi_alpha, cv->level, cv->alpha_min}, desc->math_mode == 1, stream));
    else HIP_TRY(launch_upscale(a, desc->math_mode == 1, stream));
    return launch_finish(ctx, stream, nullptr);                                      // the records are the context's: its next launch on any stream comes behind
}

}  // namespace

extern "C" {

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

float dsrt_denoise_coverage_alpha_min(void) { return kCoverageAlphaMin; }

int dsrt_denoise_accumulated_coverage(DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtAccum* acc, int samples_done, const uint32_t* d_n, const DsrtDenoiseGuides* guides,
                                      const float* d_alpha, float alpha_min, const DsrtDenoise* dn, uint8_t* d_rgb8, float* d_f32, float* d_linear, float* d_var, void* stream_v) {
    return dsrt::guarded("dsrt_denoise_accumulated_coverage", [&]() -> int {
    const CoverageInput cv{d_alpha, alpha_min};
    return denoise_impl("dsrt_denoise_accumulated_coverage", ctx, desc, acc, samples_done, d_n, guides, nullptr, dn, d_rgb8, d_f32, d_linear, d_var, (hipStream_t)stream_v, &cv);
    });
}

int dsrt_denoise_accumulated_coverage_to_host(DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtAccum* h_acc, int samples_done, const uint32_t* h_n,
                                              const DsrtDenoiseGuides* h_guides, const float* h_alpha, float alpha_min, const DsrtDenoise* dn, uint8_t* h_rgb8, float* h_f32,
                                              float* h_linear, float* h_var) {
    return dsrt::guarded("dsrt_denoise_accumulated_coverage_to_host", [&]() -> int {
    const CoverageInput hcv{h_alpha, alpha_min};
    return denoise_to_host("dsrt_denoise_accumulated_coverage_to_host", ctx, desc, h_acc, samples_done, h_n, h_guides, nullptr, dn, h_rgb8, h_f32, h_linear, h_var, &hcv);
    });
}

// The convenience form with coverage: the samples, a DIAGONAL coverage pass whose alpha and rep channels are the alpha and the guides, the demodulated filter.
int dsrt_render_denoised_coverage_to_host(DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtCoverageDesc* cov_desc, float alpha_min, const DsrtDenoise* dn,
                                          uint8_t* h_rgb8, float* h_f32, float* h_linear, float* h_var, float* h_alpha, DsrtStats* stats) {
    return dsrt::guarded("dsrt_render_denoised_coverage_to_host", [&]() -> int {
    const char* fn = "dsrt_render_denoised_coverage_to_host";
    int spp, rc;
    if ((rc = check_render_denoised(fn, ctx, desc, dn, false, nullptr, h_rgb8 || h_f32 || h_linear || h_var, &spp))) return rc;
    DsrtCoverageDesc cd;
    dsrt_coverage_defaults(&cd);
    if (cov_desc) cd = *cov_desc;
    if (cd.pattern != DSRT_COVERAGE_DIAGONAL || cd.samples < 1 || cd.samples > 64) return accum_fail(fn, "the coverage pass must be DSRT_COVERAGE_DIAGONAL with samples in 1..64");
    if (!(alpha_min > 0.0f && alpha_min <= 1.0f)) return accum_fail(fn, "alpha_min must be > 0 and <= 1");
    if ((uintptr_t)h_alpha & 3u) return accum_fail(fn, "pointer not 4-byte aligned");
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t px = (size_t)desc->width * (size_t)desc->height;
    FrameScratch f;
    DevBuf<float> alpha;
    if ((rc = f.init(px, false, true)) || (rc = alpha.alloc(px))) return rc;
    DsrtCoverage cov{};
    cov.alpha = alpha.p; cov.rep = f.gb;
    FrameBuffers h{};
    h.rgb8 = h_rgb8; h.f32 = h_f32; h.linear = h_linear; h.var = h_var;
    DsrtStats local;
    if ((rc = staged_frame_call(h, px, true, [&](const FrameBuffers& m) -> int {
        int r;
        if ((r = dsrt_render_accumulate(ctx, desc, 0, spp, 1, &f.acc, nullptr, stats ? stats : &local))) return r;
        if ((r = dsrt_render_coverage(ctx, desc, &cd, nullptr, &cov, nullptr, nullptr))) return r;
        return dsrt_denoise_accumulated_coverage(ctx, desc, &f.acc, spp, nullptr, &f.guides, alpha.p, alpha_min, dn, (uint8_t*)m.rgb8, (float*)m.f32, (float*)m.linear,
                                                 (float*)m.var, nullptr);
    }))) return rc;
    if (h_alpha) HIP_TRY(hipMemcpy(h_alpha, alpha.p, px * sizeof(float), hipMemcpyDeviceToHost));
    return DSRT_OK;
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

int dsrt_denoise_temporal_bodies(DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtAccum* acc, int samples_done, const uint32_t* d_n, const DsrtDenoiseGuides* guides,
                                 const DsrtBodyMotion* motion, const GPUCamera* prev_camera, const float* d_history_prev, float* d_history_next, const DsrtTemporal* tp,
                                 const DsrtDenoise* dn, uint8_t* d_rgb8, float* d_f32, float* d_linear, float* d_var, float* d_prev_xy, float* d_weight, float* d_prev_position,
                                 void* stream_v) {
    return dsrt::guarded("dsrt_denoise_temporal_bodies", [&]() -> int {
    const TemporalInput t{prev_camera, d_history_prev, d_history_next, tp, d_prev_xy, d_weight, true, motion, d_prev_position};
    return denoise_impl("dsrt_denoise_temporal_bodies", ctx, desc, acc, samples_done, d_n, guides, &t, dn, d_rgb8, d_f32, d_linear, d_var, (hipStream_t)stream_v);
    });
}

int dsrt_denoise_temporal_bodies_to_host(DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtAccum* h_acc, int samples_done, const uint32_t* h_n,
                                         const DsrtDenoiseGuides* h_guides, const DsrtBodyMotion* motion, const GPUCamera* prev_camera, const float* h_history_prev,
                                         float* h_history_next, const DsrtTemporal* tp, const DsrtDenoise* dn, uint8_t* h_rgb8, float* h_f32, float* h_linear, float* h_var,
                                         float* h_prev_xy, float* h_weight, float* h_prev_position) {
    return dsrt::guarded("dsrt_denoise_temporal_bodies_to_host", [&]() -> int {
    const TemporalInput ht{prev_camera, h_history_prev, h_history_next, tp, h_prev_xy, h_weight, true, motion, h_prev_position};
    return denoise_to_host("dsrt_denoise_temporal_bodies_to_host", ctx, desc, h_acc, samples_done, h_n, h_guides, &ht, dn, h_rgb8, h_f32, h_linear, h_var);
    });
}

int dsrt_denoise_temporal_shaded(DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtAccum* acc, int samples_done, const uint32_t* d_n, const DsrtDenoiseGuides* guides,
                                 const DsrtBodyMotion* motion, const DsrtTemporalShading* shading, const GPUCamera* prev_camera, const float* d_history_prev,
                                 float* d_history_next, const DsrtTemporal* tp, const DsrtDenoise* dn, uint8_t* d_rgb8, float* d_f32, float* d_linear, float* d_var,
                                 float* d_prev_xy, float* d_weight, float* d_prev_position, uint8_t* d_status, void* stream_v) {
    return dsrt::guarded("dsrt_denoise_temporal_shaded", [&]() -> int {
    const TemporalInput t{prev_camera, d_history_prev, d_history_next, tp, d_prev_xy, d_weight, motion != nullptr, motion, d_prev_position, true, shading, d_status};
    return denoise_impl("dsrt_denoise_temporal_shaded", ctx, desc, acc, samples_done, d_n, guides, &t, dn, d_rgb8, d_f32, d_linear, d_var, (hipStream_t)stream_v);
    });
}

int dsrt_denoise_temporal_shaded_to_host(DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtAccum* h_acc, int samples_done, const uint32_t* h_n,
                                         const DsrtDenoiseGuides* h_guides, const DsrtBodyMotion* motion, const DsrtTemporalShading* shading, const GPUCamera* prev_camera,
                                         const float* h_history_prev, float* h_history_next, const DsrtTemporal* tp, const DsrtDenoise* dn, uint8_t* h_rgb8, float* h_f32,
                                         float* h_linear, float* h_var, float* h_prev_xy, float* h_weight, float* h_prev_position, uint8_t* h_status) {
    return dsrt::guarded("dsrt_denoise_temporal_shaded_to_host", [&]() -> int {
    const TemporalInput ht{prev_camera, h_history_prev, h_history_next, tp, h_prev_xy, h_weight, motion != nullptr, motion, h_prev_position, true, shading, h_status};
    return denoise_to_host("dsrt_denoise_temporal_shaded_to_host", ctx, desc, h_acc, samples_done, h_n, h_guides, &ht, dn, h_rgb8, h_f32, h_linear, h_var);
    });
}

int dsrt_ctx_set_temporal_shading(DsrtContext* ctx, int mode) {
    if (!ctx) { set_error("dsrt_ctx_set_temporal_shading: null context"); return DSRT_ERR_INVALID; }
    if (mode < 0 || mode > 2) { set_error("dsrt_ctx_set_temporal_shading: mode must be 0 (off), 1 (the tap test) or 2 (with the edge guards)"); return DSRT_ERR_INVALID; }
    ctx->tp_shading = mode;
    return DSRT_OK;
}

int dsrt_ctx_temporal_shading(const DsrtContext* ctx) { return ctx ? ctx->tp_shading : 0; }

int dsrt_ctx_set_temporal_bodies(DsrtContext* ctx, int on) {
    if (!ctx) { set_error("dsrt_ctx_set_temporal_bodies: null context"); return DSRT_ERR_INVALID; }
    ctx->tp_bodies = on != 0;
    return DSRT_OK;
}

int dsrt_ctx_temporal_bodies(const DsrtContext* ctx) { return ctx && ctx->tp_bodies ? 1 : 0; }

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
    // with dsrt_ctx_set_temporal_bodies and a scene that has bodies: the motion stage, cur = the resident scene's poses, prev = this context's last temporal frame's
    BodiesResident* bd = ctx->tp_bodies && ctx->scene->bodies ? ctx->scene->bodies.get() : nullptr;
    FrameScratch f;
    const int shading_mode = ctx->tp_shading;                                         // with dsrt_ctx_set_temporal_shading: the G-buffer's flags as well, and the stage that follows shading
    if ((rc = f.init(px, false, true, bd != nullptr, shading_mode != 0))) return rc;
    if (fresh) ctx->tp_valid = false;                                                 // (growing does not keep the contents: a sequence of another size is over either way)
    for (DevBuf<float4>& h : ctx->tp_hist) if ((rc = h.grow(px * 4))) return rc;      // (only this call, which is synchronous, uses them: nothing in flight reads them)
    const GPUCamera camera = ctx->frame.camera, prev_camera = ctx->tp_camera;
    float poses_cur[kMaxBodies * 12];
    DsrtBodyMotion motion{};
    if (bd) {
        std::memcpy(poses_cur, bd->host_poses, sizeof poses_cur);
        motion = DsrtBodyMotion{bd->n_bodies, bd->first_tri.data(), bd->num_tris.data(), fresh ? poses_cur : ctx->tp_poses, poses_cur, f.prim_id.p};
    }
    const DsrtTemporalShading shading{f.flags.p, shading_mode == 2 ? 1 : 0};
    const TemporalInput t{fresh ? nullptr : &prev_camera, fresh ? nullptr : (const float*)ctx->tp_hist[ctx->tp_cur].p, (float*)ctx->tp_hist[fresh ? 0 : ctx->tp_cur ^ 1].p, tp,
                          nullptr, nullptr, bd != nullptr, bd ? &motion : nullptr, nullptr, shading_mode != 0, shading_mode ? &shading : nullptr, nullptr};
    if ((rc = render_denoised_to_host(ctx, desc, spp, f, &t, dn, h_rgb8, h_f32, h_linear, h_var, h_prev_xy, stats))) return rc;
    ctx->tp_cur = fresh ? 0 : ctx->tp_cur ^ 1;
    if (ctx->scene->bodies) std::memcpy(ctx->tp_poses, ctx->scene->bodies->host_poses, sizeof ctx->tp_poses);      // (whatever the switch says now: it may be set before the next frame)
    ctx->tp_camera = camera; ctx->tp_width = desc->width; ctx->tp_height = desc->height;
    ctx->tp_valid = true;
    return DSRT_OK;
    });
}

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

// ---- The upscaler with coverage (include/dsrt.h, COVERAGE-AWARE UPSCALER): the same calls with the two alphas, alpha_min and the level output ----
float dsrt_upscale_coverage_alpha_min(void) { return kUpscaleCoverageAlphaMin; }

int dsrt_upscale_guided_coverage(DsrtContext* ctx, const DsrtRenderDesc* desc, int lo_width, int lo_height, const float* d_lo_linear, const float* d_lo_var,
                                 const DsrtUpscaleGuides* lo, const DsrtUpscaleGuides* hi, const float* d_lo_alpha, const float* d_hi_alpha, float alpha_min,
                                 const DsrtUpscale* up, uint8_t* d_rgb8, float* d_f32, float* d_linear, float* d_var, float* d_support, uint8_t* d_level, void* stream_v) {
    return dsrt::guarded("dsrt_upscale_guided_coverage", [&]() -> int {
    const UpscaleCoverageInput cv{d_lo_alpha, d_hi_alpha, alpha_min, d_level};
    return upscale_impl("dsrt_upscale_guided_coverage", ctx, desc, lo_width, lo_height, d_lo_linear, d_lo_var, lo, hi, up, d_rgb8, d_f32, d_linear, d_var, d_support,
                        (hipStream_t)stream_v, &cv);
    });
}

int dsrt_upscale_guided_coverage_to_host(DsrtContext* ctx, const DsrtRenderDesc* desc, int lo_width, int lo_height, const float* h_lo_linear, const float* h_lo_var,
                                         const DsrtUpscaleGuides* h_lo, const DsrtUpscaleGuides* h_hi, const float* h_lo_alpha, const float* h_hi_alpha, float alpha_min,
                                         const DsrtUpscale* up, uint8_t* h_rgb8, float* h_f32, float* h_linear, float* h_var, float* h_support, uint8_t* h_level) {
    return dsrt::guarded("dsrt_upscale_guided_coverage_to_host", [&]() -> int {
    const char* fn = "dsrt_upscale_guided_coverage_to_host";
    const UpscaleCoverageInput hcv{h_lo_alpha, h_hi_alpha, alpha_min, h_level};
    if (int rc = check_upscale(fn, ctx, desc, lo_width, lo_height, h_lo_linear, h_lo_var, h_lo, h_hi, up, h_rgb8, h_f32, h_linear, h_var, h_support, &hcv)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    const FrameBuffers h = upscale_buffers(h_lo_linear, h_lo_var, *h_lo, *h_hi, h_rgb8, h_f32, h_linear, h_var, h_support, &hcv);
    return staged_frame_call(h, (size_t)desc->width * desc->height, true, [&](const FrameBuffers& m) {
        const DsrtUpscaleGuides lo = lo_guides_of(m), hi = hi_guides_of(m);
        const UpscaleCoverageInput cv{(const float*)m.lo_alpha, (const float*)m.alpha, alpha_min, (uint8_t*)m.level};
        return upscale_impl(fn, ctx, desc, lo_width, lo_height, (const float*)m.lo_linear, (const float*)m.lo_var, &lo, &hi, up, (uint8_t*)m.rgb8, (float*)m.f32, (float*)m.linear,
                            (float*)m.var, (float*)m.support, nullptr, &cv);
    }, (size_t)lo_width * lo_height);
    });
}

// The convenience form with coverage: the five calls of include/dsrt.h; both rasters' alphas and representatives' guides are on the device for the call.
int dsrt_render_upscaled_coverage_to_host(DsrtContext* ctx, const DsrtRenderDesc* lo_desc, int out_width, int out_height, const DsrtCoverageDesc* cov_lo,
                                          const DsrtCoverageDesc* cov_hi, float alpha_min, const DsrtDenoise* denoise, const DsrtUpscale* up, uint8_t* h_rgb8, float* h_f32,
                                          float* h_linear, float* h_var, uint8_t* h_lo_rgb8, float* h_alpha_hi, DsrtStats* stats) {
    return dsrt::guarded("dsrt_render_upscaled_coverage_to_host", [&]() -> int {
    const char* fn = "dsrt_render_upscaled_coverage_to_host";
    DsrtDenoise dn;
    dsrt_denoise_defaults(&dn);
    if (denoise) dn = *denoise; else dn.iterations = 0;
    int spp, rc;
    if (!ctx || !lo_desc) return accum_fail(fn, "null argument");
    DsrtRenderDesc hi_desc = *lo_desc;
    hi_desc.width = out_width; hi_desc.height = out_height;
    if ((rc = check_frame_desc(fn, lo_desc, false, true)) || (rc = check_frame_desc(fn, &hi_desc, false, true))) return rc;
    if ((rc = check_upscale_sizes(fn, lo_desc->width, lo_desc->height, out_width, out_height)) || (rc = check_upscale_params(fn, up))) return rc;
    DsrtCoverageDesc cd[2];
    const DsrtCoverageDesc* given[2] = {cov_lo, cov_hi};
    for (int k = 0; k < 2; ++k) {
        dsrt_coverage_defaults(&cd[k]);
        if (given[k]) cd[k] = *given[k];
        if (cd[k].pattern != DSRT_COVERAGE_DIAGONAL || cd[k].samples < 1 || cd[k].samples > 64) return accum_fail(fn, "the coverage passes must be DSRT_COVERAGE_DIAGONAL with samples in 1..64");
    }
    if (!(alpha_min > 0.0f && alpha_min <= 1.0f)) return accum_fail(fn, "alpha_min must be > 0 and <= 1");
    if ((uintptr_t)h_alpha_hi & 3u) return accum_fail(fn, "pointer not 4-byte aligned");
    if ((rc = check_render_denoised(fn, ctx, lo_desc, &dn, false, nullptr, h_rgb8 || h_f32 || h_linear || h_var, &spp))) return rc;      // (the scene is looked for last)
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t px_lo = (size_t)lo_desc->width * (size_t)lo_desc->height, px = (size_t)out_width * (size_t)out_height;
    FrameScratch f, g;                                                    // f: the low-resolution frame's sums and guides; g: the output raster's guides (its sums are not used)
    DevBuf<float> lo_linear, lo_var, lo_alpha, hi_alpha;
    DevBuf<uint8_t> lo_flags, hi_flags;
    if ((rc = f.init(px_lo, false, true)) || (rc = lo_linear.alloc(px_lo * 3)) || (rc = lo_var.alloc(px_lo * 3)) || (rc = lo_flags.alloc(px_lo)) || (rc = lo_alpha.alloc(px_lo))) return rc;
    if ((rc = g.normal.alloc(px * 3)) || (rc = g.position.alloc(px * 3)) || (rc = g.albedo.alloc(px * 3)) || (rc = g.range.alloc(px)) || (rc = hi_flags.alloc(px)) ||
        (rc = hi_alpha.alloc(px))) return rc;
    f.gb.flags = lo_flags.p;
    g.gb.normal = g.normal.p; g.gb.position = g.position.p; g.gb.albedo = g.albedo.p; g.gb.range = g.range.p; g.gb.flags = hi_flags.p;
    DsrtCoverage cv_lo{}, cv_hi{};
    cv_lo.alpha = lo_alpha.p; cv_lo.rep = f.gb;
    cv_hi.alpha = hi_alpha.p; cv_hi.rep = g.gb;
    const DsrtUpscaleGuides lo{f.normal.p, f.position.p, f.albedo.p, f.range.p, lo_flags.p}, hi{g.normal.p, g.position.p, g.albedo.p, g.range.p, hi_flags.p};
    FrameBuffers h{};
    h.rgb8 = h_rgb8; h.f32 = h_f32; h.linear = h_linear; h.var = h_var; h.lo_rgb8 = h_lo_rgb8;
    DsrtStats local;
    if ((rc = staged_frame_call(h, px, true, [&](const FrameBuffers& m) -> int {
        int r;
        if ((r = dsrt_render_accumulate(ctx, lo_desc, 0, spp, 1, &f.acc, nullptr, stats ? stats : &local))) return r;
        if ((r = dsrt_render_coverage(ctx, lo_desc, &cd[0], nullptr, &cv_lo, nullptr, nullptr))) return r;
        if ((r = dsrt_denoise_accumulated_coverage(ctx, lo_desc, &f.acc, spp, nullptr, &f.guides, lo_alpha.p, alpha_min, &dn, (uint8_t*)m.lo_rgb8, nullptr, lo_linear.p,
                                                   lo_var.p, nullptr))) return r;
        if ((r = dsrt_render_coverage(ctx, &hi_desc, &cd[1], nullptr, &cv_hi, nullptr, nullptr))) return r;
        return dsrt_upscale_guided_coverage(ctx, &hi_desc, lo_desc->width, lo_desc->height, lo_linear.p, lo_var.p, &lo, &hi, lo_alpha.p, hi_alpha.p, alpha_min, up,
                                            (uint8_t*)m.rgb8, (float*)m.f32, (float*)m.linear, (float*)m.var, nullptr, nullptr, nullptr);
    }, px_lo))) return rc;
    if (h_alpha_hi) HIP_TRY(hipMemcpy(h_alpha_hi, hi_alpha.p, px * sizeof(float), hipMemcpyDeviceToHost));
    return DSRT_OK;
    });
}

}  // extern "C"
