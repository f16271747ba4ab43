// api_sensor.hip -- the detector model's entry points (include/dsrt.h, SENSOR MODEL): dsrt_sensor_apply and its _to_host form.  Calls the launcher of
// sensor_kernel.hip.  The parameter defaults, the Gaussian helper and the 16-bit PNM writer need no device and live in host/sensor_host.cpp.
#include <cmath>

#include "api_internal.h"

using namespace dsrt;

namespace {

constexpr int kMaxPsfSize = 33;

size_t planes_of(const DsrtSensor* p) { return p->mono ? 1 : 3; }

// The call's four buffers, device or host form alike: the input, then the outputs as the caller gave them (one not asked for is null).
struct SensorBuffers { Staged s[4]; };
SensorBuffers sensor_buffers(size_t px, size_t planes, const float* linear, const uint16_t* dn, const float* signal, const uint8_t* rgb8) {
    return SensorBuffers{{{linear, px * 3 * sizeof(float), Dir::In}, {dn, px * planes * sizeof(uint16_t), Dir::Out}, {signal, px * planes * sizeof(float), Dir::Out},
                          {rgb8, px * 3, Dir::Out}}};
}

// Everything dsrt_sensor_apply refuses, before anything is launched or written; the same for the host form's host pointers.
int check_sensor(const char* fn, const DsrtContext* ctx, const DsrtRenderDesc* desc, const float* linear, const DsrtSensor* p, const uint16_t* dn, const float* signal,
                 const uint8_t* rgb8) {
    if (!ctx || !desc || !linear || !p) return accum_fail(fn, "null argument");
    if (desc->width < 2 || desc->height < 2) return accum_fail(fn, "width and height must be >= 2");
    if ((unsigned long long)desc->width * (unsigned long long)desc->height >= (1ull << 31)) return accum_fail(fn, "image too large (2^31 pixels)");
    if (p->psf) {
        if (p->psf_size < 1 || p->psf_size > kMaxPsfSize || !(p->psf_size & 1)) return accum_fail(fn, "psf_size must be odd and between 1 and 33");
        for (int i = 0; i < p->psf_size * p->psf_size; ++i)
            if (!(p->psf[i] >= 0.0f) || !std::isfinite(p->psf[i])) return accum_fail(fn, "a PSF tap is negative or not finite");
    }
    if (!(p->gain_e > 0.0f) || !(p->e_per_dn > 0.0f) || !(p->full_well_e > 0.0f)) return accum_fail(fn, "gain_e, e_per_dn and full_well_e must be > 0");
    if (!(p->prnu >= 0.0f) || !(p->dark_e >= 0.0f) || !(p->dsnu_e >= 0.0f) || !(p->read_e >= 0.0f)) return accum_fail(fn, "prnu, dark_e, dsnu_e and read_e must be >= 0");
    if (!std::isfinite(p->offset_dn)) return accum_fail(fn, "offset_dn must be finite");
    if (p->bits < 8 || p->bits > 16) return accum_fail(fn, "bits must be between 8 and 16");
    if (!dn && !signal && !rgb8) return accum_fail(fn, "no output");
    if (((uintptr_t)linear & 3u) || ((uintptr_t)signal & 3u)) return accum_fail(fn, "pointer not 4-byte aligned");
    if ((uintptr_t)dn & 1u) return accum_fail(fn, "the DN pointer is not 2-byte aligned");
    const SensorBuffers b = sensor_buffers((size_t)desc->width * (size_t)desc->height, planes_of(p), linear, dn, signal, rgb8);
    for (int o = 1; o < 4; ++o) {
        if (ranges_overlap(b.s[o], b.s[0])) return accum_fail(fn, "an output range overlaps the input range");
        for (int q = o + 1; q < 4; ++q) if (ranges_overlap(b.s[o], b.s[q])) return accum_fail(fn, "two output ranges overlap");
    }
    return DSRT_OK;
}

int sensor_impl(const char* fn, DsrtContext* ctx, const DsrtRenderDesc* desc, const float* d_linear, const DsrtSensor* p, uint16_t* d_dn, float* d_signal, uint8_t* d_rgb8,
                hipStream_t stream) {
    int rc;
    if ((rc = check_sensor(fn, ctx, desc, d_linear, p, d_dn, d_signal, d_rgb8))) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    if (p->psf) {
        // The taps on the device are the context's.  New taps replace them only after the context's previous launch (which may read the old ones) is over, with a
        // copy that has finished when it returns: the caller's array may go away after the call.  The same taps again -- every frame of a sequence -- upload nothing.
        const size_t taps = (size_t)p->psf_size * (size_t)p->psf_size;
        if (ctx->sn_psf_host.size() != taps || std::memcmp(ctx->sn_psf_host.data(), p->psf, taps * sizeof(float)) != 0) {
            if (ctx->done_valid) HIP_TRY(hipEventSynchronize(ctx->done));
            ctx->sn_psf_host.clear();
            if ((rc = ctx->sn_psf.grow(taps))) return rc;
            HIP_TRY(hipMemcpy(ctx->sn_psf.p, p->psf, taps * sizeof(float), hipMemcpyHostToDevice));
            ctx->sn_psf_host.assign(p->psf, p->psf + taps);
        }
    }
    if ((rc = launch_begin(ctx, stream, {}))) return rc;                             // the context's last launch (the denoiser or the upscaler that wrote d_linear) comes first
    SensorArgs a;
    std::memset(&a, 0, sizeof a);
    a.in = d_linear; a.psf = p->psf ? ctx->sn_psf.p : nullptr;
    a.out_dn = d_dn; a.out_signal = d_signal; a.out_rgb8 = d_rgb8;
    a.W = desc->width; a.H = desc->height; a.psf_size = p->psf ? p->psf_size : 1;
    a.gain_e = p->gain_e; a.prnu = p->prnu; a.dark_e = p->dark_e; a.dsnu_e = p->dsnu_e; a.read_e = p->read_e; a.full_well_e = p->full_well_e;
    a.e_per_dn = p->e_per_dn; a.offset_dn = p->offset_dn; a.bits = p->bits; a.noise = p->noise != 0;
    a.seed_lo = (uint32_t)p->seed; a.seed_hi = (uint32_t)(p->seed >> 32); a.frame = p->frame;
    HIP_TRY(launch_sensor(a, p->mono != 0, stream));
    return launch_finish(ctx, stream, nullptr);                                      // the taps are the context's: its next launch on any stream comes behind
}

}  // namespace

extern "C" {

int dsrt_sensor_apply(DsrtContext* ctx, const DsrtRenderDesc* desc, const float* d_linear, const DsrtSensor* params, uint16_t* d_dn, float* d_signal, uint8_t* d_rgb8,
                      void* stream_v) {
    return dsrt::guarded("dsrt_sensor_apply", [&]() -> int {
    return sensor_impl("dsrt_sensor_apply", ctx, desc, d_linear, params, d_dn, d_signal, d_rgb8, (hipStream_t)stream_v);
    });
}

int dsrt_sensor_apply_to_host(DsrtContext* ctx, const DsrtRenderDesc* desc, const float* h_linear, const DsrtSensor* params, uint16_t* h_dn, float* h_signal, uint8_t* h_rgb8) {
    return dsrt::guarded("dsrt_sensor_apply_to_host", [&]() -> int {
    const char* fn = "dsrt_sensor_apply_to_host";
    if (int rc = check_sensor(fn, ctx, desc, h_linear, params, h_dn, h_signal, h_rgb8)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    const SensorBuffers h = sensor_buffers((size_t)desc->width * (size_t)desc->height, planes_of(params), h_linear, h_dn, h_signal, h_rgb8);
    return staged_call(h.s, [&](void* const* m) -> int {
        if (int rc = sensor_impl(fn, ctx, desc, (const float*)m[0], params, (uint16_t*)m[1], (float*)m[2], (uint8_t*)m[3], nullptr)) return rc;
        HIP_TRY(hipStreamSynchronize(nullptr));
        return DSRT_OK;
    });
    });
}

}  // extern "C"
