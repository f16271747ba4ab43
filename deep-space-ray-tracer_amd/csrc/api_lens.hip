// api_lens.hip -- the lens model's entry points (include/dsrt.h, LENS MODEL): dsrt_lens_apply and its _to_host form.  Calls the launcher of lens_kernel.hip.  The
// parameter defaults and checks, the point helper and the pinhole's intrinsics need no device and live in host/lens_host.cpp.
#include "api_internal.h"

using namespace dsrt;

namespace {

// The call's four buffers, device or host form alike: the source, then the outputs as the caller gave them (one not asked for is null).
struct LensBuffers { Staged s[4]; };
LensBuffers lens_buffers(size_t px, const void* src, const DsrtLens* p, const DsrtLensOut& out) {
    const size_t word = sizeof(uint32_t);
    return LensBuffers{{{src, (size_t)p->src_width * (size_t)p->src_height * (size_t)p->channels * word, Dir::In}, {out.image, px * (size_t)p->channels * word, Dir::Out},
                        {out.src_xy, px * 2 * sizeof(float), Dir::Out}, {out.status, px, Dir::Out}}};
}

// Everything dsrt_lens_apply refuses, before anything is launched or written; the same for the host form's host pointers.  The context is looked at last, so that
// a machine without a device can see every other refusal (tests/test_lens_host.py): a call that gets as far as "null context" has passed them all.
int check_lens(const char* fn, const DsrtContext* ctx, const DsrtRenderDesc* desc, const void* src, const DsrtLens* p, const DsrtLensOut* out) {
    if (!desc || !src || !p || !out) return accum_fail(fn, "null argument");
    if (desc->width < 2 || desc->height < 2) return accum_fail(fn, "width and height must be >= 2");
    if ((unsigned long long)desc->width * (unsigned long long)desc->height >= (1ull << 31)) return accum_fail(fn, "image too large (2^31 pixels)");
    if (int rc = check_lens_params(fn, p, true)) return rc;
    if (!out->image && !out->src_xy && !out->status) return accum_fail(fn, "no output");
    if (((uintptr_t)src & 3u) || ((uintptr_t)out->image & 3u) || ((uintptr_t)out->src_xy & 3u)) return accum_fail(fn, "pointer not 4-byte aligned");
    const LensBuffers b = lens_buffers((size_t)desc->width * (size_t)desc->height, src, p, *out);
    for (int o = 1; o < 4; ++o) {
        if (ranges_overlap(b.s[o], b.s[0])) return accum_fail(fn, "an output range overlaps the source range");
        for (int q = o + 1; q < 4; ++q) if (ranges_overlap(b.s[o], b.s[q])) return accum_fail(fn, "two output ranges overlap");
    }
    if (!ctx) return accum_fail(fn, "null context");
    return DSRT_OK;
}

int lens_impl(const char* fn, DsrtContext* ctx, const DsrtRenderDesc* desc, const void* d_src, const DsrtLens* p, const DsrtLensOut* out, hipStream_t stream) {
    int rc;
    if ((rc = check_lens(fn, ctx, desc, d_src, p, out))) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    if ((rc = launch_begin(ctx, stream, {}))) return rc;                             // the context's last launch (whatever wrote d_src) comes first
    LensArgs a;
    std::memset(&a, 0, sizeof a);
    a.src = (const uint32_t*)d_src;
    a.out_image = (uint32_t*)out->image; a.out_src_xy = out->src_xy; a.out_status = out->status;
    a.W = desc->width; a.H = desc->height; a.src_w = p->src_width; a.src_h = p->src_height;
    a.fx = p->fx; a.fy = p->fy; a.cx = p->cx; a.cy = p->cy;
    a.src_fx = p->src_fx; a.src_fy = p->src_fy; a.src_cx = p->src_cx; a.src_cy = p->src_cy;
    a.c = LensCoeffs{p->k1, p->k2, p->k3, p->p1, p->p2};
    a.v1 = p->v1; a.v2 = p->v2; a.v3 = p->v3; a.cos4 = p->cos4; a.clamp_zero = p->clamp_zero; a.fill_bits = p->fill_bits;
    HIP_TRY(launch_lens(a, p->channels, p->filter, stream));
    return launch_finish(ctx, stream, nullptr);
}

}  // namespace

extern "C" {

int dsrt_lens_apply(DsrtContext* ctx, const DsrtRenderDesc* desc, const void* d_src, const DsrtLens* params, const DsrtLensOut* out, void* stream_v) {
    return dsrt::guarded("dsrt_lens_apply", [&]() -> int {
    return lens_impl("dsrt_lens_apply", ctx, desc, d_src, params, out, (hipStream_t)stream_v);
    });
}

int dsrt_lens_apply_to_host(DsrtContext* ctx, const DsrtRenderDesc* desc, const void* h_src, const DsrtLens* params, const DsrtLensOut* h_out) {
    return dsrt::guarded("dsrt_lens_apply_to_host", [&]() -> int {
    const char* fn = "dsrt_lens_apply_to_host";
    if (int rc = check_lens(fn, ctx, desc, h_src, params, h_out)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    const LensBuffers h = lens_buffers((size_t)desc->width * (size_t)desc->height, h_src, params, *h_out);
    return staged_call(h.s, [&](void* const* m) -> int {
        const DsrtLensOut d_out{m[1], (float*)m[2], (uint8_t*)m[3]};
        if (int rc = lens_impl(fn, ctx, desc, m[0], params, &d_out, nullptr)) return rc;
        HIP_TRY(hipStreamSynchronize(nullptr));
        return DSRT_OK;
    });
    });
}

}  // extern "C"
