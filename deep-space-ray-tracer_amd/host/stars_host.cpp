// stars_host.cpp -- the parts of the star field that need no device (include/dsrt.h, POINT SOURCES): a catalogue (right ascension, declination, magnitude) as
// world directions and fluxes, and a synthetic whole-sky catalogue.  The kernels and their entry points are csrc/stars_kernel.hip and csrc/api_stars.hip.
// Both are conveniences in double precision on the C library's sin, cos, pow and log10: their bits are not part of the contract.
#include <cmath>
#include <cstdint>

#include "../../include/dsrt.h"
#include "host_internal.hpp"

// dir = (cos d cos a, cos d sin a, sin d), flux = flux_mag0 * 10^(-0.4 mag).
extern "C" int dsrt_stars_from_catalog(int n, const double* ra_deg, const double* dec_deg, const double* mag, const float flux_mag0[3], double* world_dirs, float* flux) {
    return dsrt::guarded("dsrt_stars_from_catalog", [&]() -> int {
    if (n < 0 || !flux_mag0 || (n > 0 && (!ra_deg || !dec_deg || !mag || !world_dirs || !flux))) {
        dsrt::set_error("dsrt_stars_from_catalog: n < 0 or a NULL array");
        return DSRT_ERR_INVALID;
    }
    const double rad = 3.14159265358979323846 / 180.0;
    for (int i = 0; i < n; ++i) {
        const double a = ra_deg[i] * rad, d = dec_deg[i] * rad, cd = std::cos(d);
        world_dirs[3 * i] = cd * std::cos(a); world_dirs[3 * i + 1] = cd * std::sin(a); world_dirs[3 * i + 2] = std::sin(d);
        const double s = std::pow(10.0, -0.4 * mag[i]);
        for (int k = 0; k < 3; ++k) flux[3 * i + k] = (float)((double)flux_mag0[k] * s);
    }
    return DSRT_OK;
    });
}

// splitmix64 -> doubles in [0, 1).  Uniform on the sphere: sin(dec) uniform in [-1, 1), ra uniform in [0, 360).  Magnitudes follow the sky's rough count law,
// N(< m) proportional to 10^(0.5 m), between mag_min and mag_max: most stars are faint.
extern "C" int dsrt_stars_synthetic_catalog(uint64_t seed, int n, double mag_min, double mag_max, double* ra_deg, double* dec_deg, double* mag) {
    return dsrt::guarded("dsrt_stars_synthetic_catalog", [&]() -> int {
    if (n < 0 || !(mag_min <= mag_max) || !std::isfinite(mag_min) || !std::isfinite(mag_max) || (n > 0 && (!ra_deg || !dec_deg || !mag))) {
        dsrt::set_error("dsrt_stars_synthetic_catalog: n < 0, a magnitude range that is empty or not finite, or a NULL array");
        return DSRT_ERR_INVALID;
    }
    uint64_t state = seed;
    auto next = [&]() {
        uint64_t z = (state += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return (double)((z ^ (z >> 31)) >> 11) * 0x1p-53;
    };
    const double deg = 180.0 / 3.14159265358979323846;
    const double lo = std::pow(10.0, 0.5 * mag_min), hi = std::pow(10.0, 0.5 * mag_max);
    for (int i = 0; i < n; ++i) {
        ra_deg[i] = 360.0 * next();
        dec_deg[i] = std::asin(2.0 * next() - 1.0) * deg;
        const double m = 2.0 * std::log10(lo + next() * (hi - lo));
        mag[i] = std::fmin(std::fmax(m, mag_min), mag_max);
    }
    return DSRT_OK;
    });
}
