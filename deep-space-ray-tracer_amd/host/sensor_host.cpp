// sensor_host.cpp -- the parts of the detector model that need no device (include/dsrt.h, SENSOR MODEL): the parameter defaults, the Gaussian PSF helper and the
// 16-bit PNM writer for raw DN frames.  The kernel and its entry points are csrc/sensor_kernel.hip and csrc/api_sensor.hip.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "../../include/dsrt.h"
#include "host_internal.hpp"

extern "C" void dsrt_sensor_defaults(DsrtSensor* out) {
    if (!out) return;
    std::memset(out, 0, sizeof *out);
    out->psf = nullptr; out->psf_size = 0; out->mono = 0;
    out->gain_e = 20000.0f; out->prnu = 0.0f; out->dark_e = 0.0f; out->dsnu_e = 0.0f; out->read_e = 10.0f; out->full_well_e = 20000.0f;
    out->e_per_dn = 5.0f; out->offset_dn = 64.0f; out->bits = 12;
    out->noise = 1; out->seed = 1337; out->frame = 0;
}

// exp(-(kx^2 + ky^2) / (2 sigma^2)) in double, divided by the double sum of the taps in row-major order, rounded to float.
extern "C" int dsrt_sensor_psf_gaussian(float sigma, int size, float* taps) {
    return dsrt::guarded("dsrt_sensor_psf_gaussian", [&]() -> int {
    if (!taps || size < 1 || size > 33 || !(size & 1) || !(sigma > 0.0f) || !std::isfinite(sigma)) {
        dsrt::set_error("dsrt_sensor_psf_gaussian: size must be odd and between 1 and 33, sigma > 0 and finite, taps not NULL");
        return DSRT_ERR_INVALID;
    }
    const int r = (size - 1) / 2;
    const double two_s2 = 2.0 * (double)sigma * (double)sigma;
    std::vector<double> g((size_t)size * (size_t)size);
    double sum = 0.0;
    for (int ky = -r; ky <= r; ++ky)
        for (int kx = -r; kx <= r; ++kx) {
            const double v = std::exp(-(double)(kx * kx + ky * ky) / two_s2);
            g[(size_t)(ky + r) * (size_t)size + (size_t)(kx + r)] = v;
            sum += v;
        }
    for (size_t i = 0; i < g.size(); ++i) taps[i] = (float)(g[i] / sum);
    return DSRT_OK;
    });
}

// P5 (one channel) or P6 (three), rows top-down as the format has them.  maxval > 255 (every ADC but the 8-bit one): two bytes per sample, most significant first;
// otherwise one byte per sample, which is what the format prescribes for such a maxval.
extern "C" int dsrt_write_pnm16(const char* path, const uint16_t* dn, int width, int height, int channels, int maxval) {
    return dsrt::guarded("dsrt_write_pnm16", [&]() -> int {
    if (!path || !dn || width <= 0 || height <= 0 || (channels != 1 && channels != 3) || maxval < 1 || maxval > 65535) {
        dsrt::set_error("dsrt_write_pnm16: bad argument (channels 1 or 3, maxval between 1 and 65535)");
        return DSRT_ERR_INVALID;
    }
    const size_t row = (size_t)width * (size_t)channels;
    const bool wide = maxval > 255;
    std::vector<uint8_t> bytes(row * (wide ? 2 : 1));
    FILE* f = std::fopen(path, "wb");
    if (!f) { dsrt::set_error(std::string("cannot open ") + path + " for writing"); return DSRT_ERR_IO; }
    bool ok = std::fprintf(f, "%s\n%d %d\n%d\n", channels == 3 ? "P6" : "P5", width, height, maxval) > 0;
    for (int y = 0; y < height && ok; ++y) {
        const uint16_t* src = dn + (size_t)y * row;
        for (size_t i = 0; i < row; ++i) {
            if (wide) { bytes[2 * i] = (uint8_t)(src[i] >> 8); bytes[2 * i + 1] = (uint8_t)src[i]; }
            else bytes[i] = (uint8_t)src[i];
        }
        ok = std::fwrite(bytes.data(), 1, bytes.size(), f) == bytes.size();
    }
    ok = std::fclose(f) == 0 && ok;
    if (!ok) { dsrt::set_error(std::string("short write to ") + path); return DSRT_ERR_IO; }
    return DSRT_OK;
    });
}
