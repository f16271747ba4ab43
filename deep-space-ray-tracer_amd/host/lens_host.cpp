// lens_host.cpp -- the parts of the lens model that need no device (include/dsrt.h, LENS MODEL): the parameter defaults, the checks of a DsrtLens, the forward
// model on points (labels) and the library's own pinhole intrinsics.  The arithmetic is csrc/lens_math.h's, the header the kernel compiles too; the kernel and its
// entry points are csrc/lens_kernel.hip and csrc/api_lens.hip.
#include <cmath>
#include <cstring>

#include "../../include/dsrt.h"
#include "../csrc/lens_math.h"
#include "host_internal.hpp"

namespace dsrt {

int check_lens_params(const char* fn, const DsrtLens* p, bool warp) {
    auto refuse = [&](const char* why) { set_error(std::string(fn) + ": " + why); return DSRT_ERR_INVALID; };
    for (float f : {p->fx, p->fy, p->src_fx, p->src_fy}) if (!(f > 0.0f) || !std::isfinite(f)) return refuse("fx, fy, src_fx and src_fy must be > 0 and finite");
    for (float c : {p->cx, p->cy, p->src_cx, p->src_cy}) if (!std::isfinite(c)) return refuse("a principal point is not finite");
    for (float k : {p->k1, p->k2, p->k3, p->p1, p->p2}) if (!std::isfinite(k)) return refuse("a distortion coefficient is not finite");
    if (!warp) return DSRT_OK;
    for (float v : {p->v1, p->v2, p->v3}) if (!std::isfinite(v)) return refuse("a vignetting coefficient is not finite");
    if (p->src_width < 2 || p->src_height < 2) return refuse("src_width and src_height must be >= 2");
    if ((unsigned long long)p->src_width * (unsigned long long)p->src_height >= (1ull << 31)) return refuse("source too large (2^31 pixels)");
    if (p->filter < DSRT_LENS_NEAREST || p->filter > DSRT_LENS_CUBIC) return refuse("filter must be 0 (nearest), 1 (bilinear) or 2 (Catmull-Rom)");
    if (p->channels < 1 || p->channels > 4) return refuse("channels must be between 1 and 4");
    if ((p->cos4 != 0 && p->cos4 != 1) || (p->clamp_zero != 0 && p->clamp_zero != 1)) return refuse("cos4 and clamp_zero are 0 or 1");
    return DSRT_OK;
}

}  // namespace dsrt

extern "C" void dsrt_lens_defaults(DsrtLens* out) {
    if (!out) return;
    std::memset(out, 0, sizeof *out);
    out->filter = DSRT_LENS_CUBIC; out->channels = 3; out->clamp_zero = 1;
}

extern "C" int dsrt_lens_distort_points(const DsrtLens* p, int n, const float* xy_src, float* xy_out, uint8_t* ok) {
    return dsrt::guarded("dsrt_lens_distort_points", [&]() -> int {
    const char* fn = "dsrt_lens_distort_points";
    if (!p || n < 0 || (n > 0 && (!xy_src || !xy_out))) { dsrt::set_error(std::string(fn) + ": null argument or n < 0"); return DSRT_ERR_INVALID; }
    if (int rc = dsrt::check_lens_params(fn, p, false)) return rc;
    const dsrt::LensCoeffs c{p->k1, p->k2, p->k3, p->p1, p->p2};
    for (int i = 0; i < n; ++i) {
        const float px = xy_src[2 * i], py = xy_src[2 * i + 1];
        const float xu = (px - p->src_cx) / p->src_fx, yu = (py - p->src_cy) / p->src_fy;
        float xr, yr;
        dsrt::lens_distort(c, xu, yu, xr, yr);
        const float ox = xr * p->fx + p->cx, oy = yr * p->fy + p->cy;
        const bool good = std::isfinite(px) && std::isfinite(py) && std::isfinite(ox) && std::isfinite(oy);
        xy_out[2 * i] = good ? ox : 0.0f;
        xy_out[2 * i + 1] = good ? oy : 0.0f;
        if (ok) ok[i] = good ? 1 : 0;
    }
    return DSRT_OK;
    });
}

// TEMPORAL ACCUMULATION's projection of a direction D is fx = s (W-1) - 0.5 with s = (a k - eu)/hu, k = ew/cc, and fy = (H-1) - (t (H-1) - 0.5) with
// t = (b k - ev)/vv.  With xu = -a/cc and yu = b/cc that is a k = -ew xu and b k = ew yu, hence the four numbers below.
extern "C" int dsrt_lens_intrinsics_from_camera(const GPUCamera* cam, int width, int height, float out[4]) {
    return dsrt::guarded("dsrt_lens_intrinsics_from_camera", [&]() -> int {
    const char* fn = "dsrt_lens_intrinsics_from_camera";
    if (!cam || !out || width < 2 || height < 2) { dsrt::set_error(std::string(fn) + ": null argument, or width or height < 2"); return DSRT_ERR_INVALID; }
    auto dot = [](const DsrtF3& a, const DsrtF3& b) { return (double)a.x * b.x + (double)a.y * b.y + (double)a.z * b.z; };
    const DsrtF3 e{cam->lower_left_corner.x - cam->origin.x, cam->lower_left_corner.y - cam->origin.y, cam->lower_left_corner.z - cam->origin.z};
    const double eu = dot(e, cam->u), ev = dot(e, cam->v), ew = dot(e, cam->w), hu = dot(cam->horizontal, cam->u), vv = dot(cam->vertical, cam->v);
    const double w1 = (double)(width - 1), h1 = (double)(height - 1);
    const double v[4] = {-ew * w1 / hu, -ew * h1 / vv, -eu * w1 / hu - 0.5, h1 + 0.5 + ev * h1 / vv};
    if (hu == 0.0 || vv == 0.0 || ew == 0.0 || !std::isfinite(v[0]) || !std::isfinite(v[1]) || !std::isfinite(v[2]) || !std::isfinite(v[3])) {
        dsrt::set_error(std::string(fn) + ": the camera's horizontal . u, vertical . v or (corner - origin) . w is zero or not finite");
        return DSRT_ERR_INVALID;
    }
    for (int i = 0; i < 4; ++i) out[i] = (float)v[i];
    return DSRT_OK;
    });
}
