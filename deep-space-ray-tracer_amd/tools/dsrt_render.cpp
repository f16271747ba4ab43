// dsrt_render -- frame driver over the C ABI, taking the reference executable's flags.
//
// Mirrors what src/main.cpp of the reference does per run: --input_txt <pose file>, --output_dir <dir>
// (:194-215), one frame per pose named frame_%04zu.ppm (:418-425), frames closer than 1 m skipped (:342-345),
// camera at cam_in_model looking at the model origin with vfov 40 (:254-260, :399).  Differences, all deliberate:
//   * the mesh path, image size, spp and depth are flags (--obj --width --height --spp --depth) instead of
//     constants (:238, :255-258);
//   * the scene is flattened, BVH-built and uploaded ONCE; only camera and sun change per frame (the reference
//     rebuilds and re-uploads everything per frame, :405);
//   * the output directory is created if missing but never emptied (the reference deletes its contents, :41-50);
//   * PPM (or PNG with --png): there is no ImageMagick shell-out (:28-36), and --upscale does not shell out to a learned upscaler (:194-215, :438-447): in
//     rng_mode 0 the flag is announced as unsupported and ignored; in rng_mode 1 see below;
//   * --gbuffer also writes each frame's ground truth next to it (include/dsrt.h, dsrt_render_gbuffer): <frame>_range.pfm, <frame>_normal.pfm,
//     <frame>_mask.pgm (255 where the centre ray hits) and <frame>_sunlit.pgm (255 where that hit sees the Sun).
//   * rng_mode 1 only: --passes P renders each frame as P interleaved sample sets and writes <frame>_pass<p>of<P> after each (a preview that
//     sharpens), then <frame> itself -- the last pass's image, byte for byte the one-launch image; --variance also writes the variance of every
//     pixel's mean as <frame>_var.pfm (include/dsrt.h, SAMPLE SETS).
//   * rng_mode 1 only: --adaptive TOL renders each frame with adaptive sampling (include/dsrt.h, ADAPTIVE SAMPLING: dsrt_render_adaptive) -- up to
//     --adaptive-passes P (8) interleaved passes, the first --adaptive-min-passes M (2) over every pixel, the later ones over the pixels whose standard error
//     still exceeds TOL times their mean (or times --adaptive-floor F, for dark pixels) -- and writes <frame> and <frame>_spp.pfm, every pixel's sample count
//     (with --variance also <frame>_var.pfm).
//   * rng_mode 1 only: --denoise [ITER] reconstructs each frame from its samples with the variance-guided a-trous filter (include/dsrt.h, DENOISER: the
//     library's default parameters, ITER iterations if given) -- the reference's reconstruction step runs outside its renderer (scripts/upsample.py) -- and
//     writes <frame> denoised and <frame>_raw undenoised, byte for byte the frame without the flag (with --variance also <frame>_var.pfm, the
//     filtered image's propagated variance).
//   * with --denoise: --temporal carries every frame's accumulated mean and variance on to the next, reprojected through the previous camera (include/dsrt.h,
//     TEMPORAL ACCUMULATION: dsrt_render_denoised_temporal_to_host, the library's default parameters).  Frames are rendered in pose order, a skipped frame leaves the
//     history as it is, and frame i (its index in the pose file) is rendered with seed 1337 + i: the blend takes the frames' noise as independent, which one seed for
//     all frames would not give.  <frame>_raw is that frame's own samples, undenoised.  --flow also writes <frame>_flow.pfm: per pixel where its surface point was
//     in the previous frame, as (fx - x, fy - y, 0) in pixels (NaN where it was not in view, and in the first frame) -- optical-flow ground truth.
//   * rng_mode 1 only: --upscale [S] (S = 2 .. 8, default 4, the reference's default scale) renders each frame at --width x --height and reconstructs it at
//     S*width x S*height with the G-buffer-guided upscaler (include/dsrt.h, UPSCALER: dsrt_render_upscaled_to_host, the library's default parameters): the
//     full-resolution G-buffer of the same camera keeps silhouettes, creases, material edges and sun-shadow edges at the output resolution.  Writes <frame> at the
//     output size and <frame>_lowres, byte for byte the frame the same command writes without --upscale.  With --denoise [ITER] the denoiser runs between the two
//     steps; --variance writes the upscaled variance as <frame>_var.pfm.  Does not combine with --temporal, --adaptive, --passes or --gbuffer.
//   * --body OBJ [--body-scale S] (repeatable, up to 15) adds a MOVABLE RIGID BODY (include/dsrt.h, MOVABLE RIGID BODIES) and --body-poses FILE poses them: one
//     line per RENDERED frame, 12 numbers per body (row-major 3x4 [R | t] in the model frame, applied to the body's rest pose; '#' lines are comments; frames past
//     the last line keep the last poses).  The scene is uploaded once with dsrt_scene_upload_bodies and posed on the device before each frame; a batch launch has
//     one set of poses, so such a run renders one launch per frame.  Does not combine with --bvh sah|lbvh, --fast or --certified-tree.
//     With --denoise --temporal a pose update starts the history afresh unless --follow-bodies is given: then the history follows the bodies (include/dsrt.h,
//     TEMPORAL ACCUMULATION WITH BODIES: dsrt_ctx_set_temporal_bodies), and --flow is flow ground truth that includes their motion.
//   * --follow-shading (with --denoise --temporal, with or without --follow-bodies): the history keeps every surface point's sun state and gives up what lies across
//     or next to a moved shadow edge (include/dsrt.h, TEMPORAL ACCUMULATION THAT FOLLOWS SHADING: dsrt_ctx_set_temporal_shading, mode 2).
//   * --coverage grid:S|diag:N also writes each frame's sub-pixel coverage (include/dsrt.h, COVERAGE: dsrt_render_coverage; S x S sub-samples on a grid, S = 1 .. 8,
//     or N = 1 .. 64 along the pixel's diagonal), in either rng_mode and beside any other mode: <frame>_alpha.pfm, the share of the sub-samples that hit (a soft mask),
//     <frame>_sun_alpha.pfm, the share that hit and see the Sun (an antialiased shadow mask), and with --body <frame>_body_alpha.pfm: one plane per body, the static
//     part first, stacked top to bottom in one single-channel map of height (bodies + 1) * H -- the share of the sub-samples that hit that body.
//   * with --denoise: --coverage-aware [ALPHA_MIN] filters the covered part of every pixel (include/dsrt.h, COVERAGE DEMODULATION: a DIAGONAL 64 coverage pass gives
//     alpha and the guides, dsrt_denoise_accumulated_coverage; ALPHA_MIN in (0, 1], default the library's), so that silhouette pixels and trusses thinner than a
//     pixel are filtered too.  Does not combine with --temporal.
//   * rng_mode 1 only: --upscale [S] --coverage-aware [ALPHA_MIN] [--coverage diag:N] is the upscaler with coverage (include/dsrt.h, COVERAGE-AWARE UPSCALER:
//     dsrt_render_upscaled_coverage_to_host): a DIAGONAL N coverage pass at each raster (default 64; a grid: pattern is a usage error) gives the alphas and the
//     guides (ALPHA_MIN: default the library's for this chain), the low-resolution frame is unmixed before the gather, and trusses thinner than a low-resolution pixel come out at the output resolution.  Writes
//     <frame>, <frame>_lowres and <frame>_alpha.pfm (the output raster's alpha); --coverage then only chooses N and writes no files of its own.  The three flags
//     --denoise --upscale --coverage-aware together stay a usage error: the low-resolution frame of this mode is the plain mean.
//   * rng_mode 1 only: --sensor SPEC degrades each frame's LINEAR image into what a camera would have delivered (include/dsrt.h, SENSOR MODEL: dsrt_sensor_apply_to_host)
//     and writes <frame>_raw.pgm (mono) or <frame>_raw.ppm, the raw DN frame with maxval 2^bits - 1 (two bytes per sample, most significant first, above 8 bits), and
//     <frame>_sensor.png, its top eight bits.  SPEC is a comma list, every key optional, the rest the library's defaults:
//       psf=gauss:SIGMA:SIZE | psf=FILE.pfm (one channel, odd square size up to 33)   gain=  read=  dark=  prnu=  dsnu=  well=  epdn=  offset=  bits=  mono  noise=0|1  seed=
//     e.g. psf=gauss:1.2:9,gain=20000,read=12,dark=3,prnu=0.01,dsnu=2,well=20000,epdn=5,offset=64,bits=12,mono,seed=7.  A malformed SPEC is a usage error before any
//     device is touched.  The linear image is the chosen chain's: the denoiser's (--denoise, with or without --temporal or --coverage-aware), the upscaler's
//     (--upscale: the raw frame then has the output size), and without either the plain mean (dsrt_render_denoised_to_host with 0 iterations).  The detector's
//     `frame` is the frame's index in the pose file, so in a sequence the fixed pattern (prnu, dsnu) stays put while the temporal noise changes.  With --denoise the
//     undenoised image is then called <frame>_noisy: _raw is the detector's.  In rng_mode 0 the flag is announced and ignored, like --upscale.  Does not combine with
//     --adaptive, --passes or --gbuffer.
//   * rng_mode 1 only: --stars FILE[,flux=F][,occlusion=0] adds a star field to each frame's LINEAR image (include/dsrt.h, POINT SOURCES: dsrt_render_stars_to_host).
//     FILE holds one `ra_deg dec_deg mag` per line (blank lines and lines that begin with # are skipped); a star's flux is F * 10^(-0.4 mag) in all three channels
//     (F: default 1, linear signal x pixel of a magnitude-0 star); occlusion=0 draws the stars through the scene.  Per frame the catalogue's directions go through
//     that frame's pose (dsrt_pose_dirs_to_model), and the layer is added to the chain's linear image -- after the denoiser or the upscaler, at the output size, and
//     before --sensor, whose raw frame then contains the stars.  Writes <frame>_stars.pfm (the layer) and <frame>_stars.txt (per star: index, fx, fy, status);
//     without --sensor nothing else changes.  A malformed spec or catalogue is a usage error before any device is touched.  In rng_mode 0 the flag is announced and
//     ignored, like --sensor; it refuses the combinations --sensor refuses.
//   * rng_mode 1 only: --lens SPEC warps each frame's LINEAR image through a lens (include/dsrt.h, LENS MODEL: dsrt_lens_apply_to_host).  SPEC is a comma list, every
//     key optional:  k1=  k2=  k3=  p1=  p2=  (Brown-Conrady)   zoom=Z (the output's focal length is Z times the frame's; default 1)   vig=V1:V2:V3   cos4
//     filter=nearest|linear|cubic (default cubic).  The source is the chain's linear image with the intrinsics of the frame's camera
//     (dsrt_lens_intrinsics_from_camera); the output has the same size and principal point.  It runs after --stars and before --sensor, whose raw frame is then the
//     distorted one.  Writes <frame>_lens.pfm (the warped linear image), <frame>_lens_map.pfm (three channels: the source position sx, sy and the status byte) and,
//     with --stars, <frame>_stars_lens.txt (per star: index, its centroid in the distorted frame -- dsrt_lens_distort_points of <frame>_stars.txt's -- and the
//     star's status; a star that was not projected keeps 0 0).  Without --lens every other file is byte for byte what it is without this flag.  A malformed SPEC is
//     a usage error before any device is touched.  In rng_mode 0 the flag is announced and ignored, like --sensor; it refuses the combinations --sensor refuses.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <fstream>
#include <sstream>
#include <string>
#include <sys/stat.h>
#include <vector>

#include "../../include/dsrt.h"

// 8-bit P5 of `bit` of every flags byte: 255 where set
static bool write_mask_pgm(const std::string& path, const std::vector<uint8_t>& flags, int width, int height, uint8_t bit) {
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    std::vector<uint8_t> px(flags.size());
    for (size_t i = 0; i < flags.size(); ++i) px[i] = (flags[i] & bit) ? 255 : 0;
    bool ok = std::fprintf(f, "P5\n%d %d\n255\n", width, height) > 0 && std::fwrite(px.data(), 1, px.size(), f) == px.size();
    return std::fclose(f) == 0 && ok;
}

// --sensor SPEC (include/dsrt.h, SENSOR MODEL): the library's defaults with the SPEC's keys applied, and the taps the psf key made.  Everything dsrt_sensor_apply
// would refuse of the parameters is refused here already, with `why` saying what: the CLI then ends before a device context exists.
struct SensorSpec { DsrtSensor p; std::vector<float> taps; };

// A one-channel PFM ("Pf", rows bottom-up, a negative scale = little-endian) of odd square size as row-major taps, top row first.
static bool read_psf_pfm(const std::string& path, std::vector<float>& taps, int& size, std::string& why) {
    std::ifstream in(path, std::ios::binary);
    if (!in) { why = "cannot open " + path; return false; }
    std::string magic;
    int w = 0, h = 0;
    double scale = 0.0;
    if (!(in >> magic >> w >> h >> scale) || magic != "Pf" || scale == 0.0) { why = path + " is not a one-channel PFM (Pf)"; return false; }
    if (w != h || !(w & 1) || w < 1 || w > 33) { why = path + ": a PSF is square, of odd size between 1 and 33"; return false; }
    in.get();                                                      // the single white-space byte after the scale
    std::vector<uint8_t> bytes((size_t)w * h * 4);
    if (!in.read((char*)bytes.data(), (std::streamsize)bytes.size())) { why = path + " is shorter than its header says"; return false; }
    taps.resize((size_t)w * h);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const uint8_t* b = bytes.data() + ((size_t)(h - 1 - y) * w + x) * 4;
            const uint32_t u = scale < 0.0 ? (uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24
                                           : (uint32_t)b[3] | (uint32_t)b[2] << 8 | (uint32_t)b[1] << 16 | (uint32_t)b[0] << 24;
            std::memcpy(&taps[(size_t)y * w + x], &u, 4);
        }
    size = w;
    return true;
}

// --stars FILE[,flux=F][,occlusion=0] (include/dsrt.h, POINT SOURCES): the catalogue as world directions and fluxes.
struct StarsSpec { std::vector<double> world_dirs; std::vector<float> flux; int occlusion = 1; };

static bool parse_stars_spec(const std::string& spec, StarsSpec& out, std::string& why) {
    std::vector<std::string> parts;
    for (size_t at = 0;;) {
        const size_t comma = spec.find(',', at);
        parts.push_back(spec.substr(at, comma == std::string::npos ? std::string::npos : comma - at));
        if (comma == std::string::npos) break;
        at = comma + 1;
    }
    if (parts[0].empty()) { why = "FILE[,flux=F][,occlusion=0|1]: no FILE"; return false; }
    double flux0 = 1.0;
    for (size_t k = 1; k < parts.size(); ++k) {
        const size_t eq = parts[k].find('=');
        const std::string key = parts[k].substr(0, eq), v = eq == std::string::npos ? "" : parts[k].substr(eq + 1);
        char* end = nullptr;
        const double x = std::strtod(v.c_str(), &end);
        if (v.empty() || *end) { why = "`" + parts[k] + "` is not key=number"; return false; }
        if (key == "flux") { if (!(x >= 0.0) || !std::isfinite(x)) { why = "flux must be >= 0 and finite"; return false; } flux0 = x; }
        else if (key == "occlusion") { if (x != 0.0 && x != 1.0) { why = "occlusion is 0 or 1"; return false; } out.occlusion = (int)x; }
        else { why = "unknown key `" + key + "` (flux, occlusion)"; return false; }
    }
    std::ifstream in(parts[0]);
    if (!in) { why = "cannot open " + parts[0]; return false; }
    std::vector<double> ra, dec, mag;
    std::string line;
    while (std::getline(in, line)) {
        const size_t start = line.find_first_not_of(" \t\r");
        if (start == std::string::npos || line[start] == '#') continue;
        std::istringstream is(line);
        double a, d, m;
        std::string rest;
        if (!(is >> a >> d >> m) || (is >> rest) || !std::isfinite(a) || !std::isfinite(d) || !std::isfinite(m)) {
            why = parts[0] + ": line " + std::to_string(ra.size() + 1) + " of the catalogue is not `ra_deg dec_deg mag`"; return false;
        }
        ra.push_back(a); dec.push_back(d); mag.push_back(m);
    }
    if (ra.size() > ((size_t)1 << 22)) { why = parts[0] + " holds more than 2^22 stars"; return false; }
    const float f3[3] = {(float)flux0, (float)flux0, (float)flux0};
    out.world_dirs.resize(ra.size() * 3); out.flux.resize(ra.size() * 3);
    if (dsrt_stars_from_catalog((int)ra.size(), ra.data(), dec.data(), mag.data(), f3, out.world_dirs.data(), out.flux.data()) != DSRT_OK) { why = dsrt_last_error(); return false; }
    return true;
}

// --lens SPEC (include/dsrt.h, LENS MODEL): the library's defaults with the SPEC's keys applied; the two frames are set per frame, from its camera.
struct LensSpec { DsrtLens p; double zoom = 1.0; };

static bool parse_lens_spec(const std::string& spec, LensSpec& out, std::string& why) {
    static const char* known = "k1 k2 k3 p1 p2 zoom vig cos4 filter";
    dsrt_lens_defaults(&out.p);
    auto number = [&](const std::string& key, const std::string& v, double& x) {
        char* end = nullptr;
        x = std::strtod(v.c_str(), &end);
        if (v.empty() || *end || !std::isfinite(x) || !std::isfinite((float)x)) { why = key + " needs a finite number, not '" + v + "'"; return false; }
        return true;
    };
    if (spec.empty()) { why = "an empty SPEC"; return false; }
    size_t at = 0;
    while (at <= spec.size()) {
        const size_t comma = std::min(spec.find(',', at), spec.size());
        const std::string item = spec.substr(at, comma - at);
        at = comma + 1;
        const size_t eq = item.find('=');
        const std::string key = item.substr(0, eq), v = eq == std::string::npos ? "" : item.substr(eq + 1);
        double x = 0.0;
        if (key == "cos4" && eq == std::string::npos) out.p.cos4 = 1;
        else if (eq == std::string::npos) { why = item.empty() ? "an empty item" : "'" + item + "' needs a value (key=value); known keys: " + known; return false; }
        else if (key == "filter") {
            if (v == "nearest") out.p.filter = DSRT_LENS_NEAREST;
            else if (v == "linear") out.p.filter = DSRT_LENS_BILINEAR;
            else if (v == "cubic") out.p.filter = DSRT_LENS_CUBIC;
            else { why = "filter is nearest, linear or cubic, not '" + v + "'"; return false; }
        }
        else if (key == "vig") {
            const size_t c1 = v.find(':'), c2 = c1 == std::string::npos ? c1 : v.find(':', c1 + 1);
            double a = 0.0, b = 0.0, c = 0.0;
            if (c2 == std::string::npos || !number("vig=V1", v.substr(0, c1), a) || !number("vig=V1:V2", v.substr(c1 + 1, c2 - c1 - 1), b) || !number("vig=V1:V2:V3", v.substr(c2 + 1), c)) {
                if (why.empty()) why = "vig takes V1:V2:V3";
                return false;
            }
            out.p.v1 = (float)a; out.p.v2 = (float)b; out.p.v3 = (float)c;
        }
        else if (!number(key, v, x)) return false;
        else if (key == "k1") out.p.k1 = (float)x;
        else if (key == "k2") out.p.k2 = (float)x;
        else if (key == "k3") out.p.k3 = (float)x;
        else if (key == "p1") out.p.p1 = (float)x;
        else if (key == "p2") out.p.p2 = (float)x;
        else if (key == "zoom") { if (!(x > 0.0)) { why = "zoom must be > 0"; return false; } out.zoom = x; }
        else if (key == "cos4") { if (x != 0.0 && x != 1.0) { why = "cos4 is 0 or 1"; return false; } out.p.cos4 = (int)x; }
        else { why = "unknown key '" + key + "'; known keys: " + known; return false; }
    }
    return true;
}

static bool parse_sensor_spec(const std::string& spec, SensorSpec& out, std::string& why) {
    dsrt_sensor_defaults(&out.p);
    auto number = [&](const std::string& key, const std::string& v, double& x) {
        char* end = nullptr;
        x = std::strtod(v.c_str(), &end);
        if (v.empty() || *end) { why = key + " needs a number, not '" + v + "'"; return false; }
        return true;
    };
    if (spec.empty()) { why = "an empty SPEC"; return false; }
    size_t at = 0;
    while (at <= spec.size()) {
        const size_t comma = std::min(spec.find(',', at), spec.size());
        const std::string item = spec.substr(at, comma - at);
        at = comma + 1;
        const size_t eq = item.find('=');
        const std::string key = item.substr(0, eq), v = eq == std::string::npos ? "" : item.substr(eq + 1);
        double x = 0.0;
        if (key == "mono" && eq == std::string::npos) out.p.mono = 1;
        else if (eq == std::string::npos) { why = item.empty() ? "an empty item" : "'" + item + "' needs a value (key=value); known keys: psf gain read dark prnu dsnu well epdn offset bits mono noise seed"; return false; }
        else if (key == "psf") {
            int size = 0;
            if (v.rfind("gauss:", 0) == 0) {
                const size_t colon = v.find(':', 6);
                double sigma = 0.0, n = 0.0;
                if (colon == std::string::npos || !number("psf=gauss:SIGMA", v.substr(6, colon - 6), sigma) || !number("psf=gauss:SIGMA:SIZE", v.substr(colon + 1), n)) {
                    if (why.empty()) why = "psf=gauss takes SIGMA:SIZE";
                    return false;
                }
                size = (int)n;
                if ((double)size != n || size < 1 || size > 33 || !(size & 1)) { why = "psf=gauss:SIGMA:SIZE needs an odd SIZE between 1 and 33"; return false; }
                out.taps.resize((size_t)size * size);
                if (dsrt_sensor_psf_gaussian((float)sigma, size, out.taps.data()) != DSRT_OK) { why = "psf=gauss:SIGMA:SIZE needs SIGMA > 0"; return false; }
            } else if (!read_psf_pfm(v, out.taps, size, why)) return false;
            for (float t : out.taps) if (!(t >= 0.0f) || !std::isfinite(t)) { why = "a PSF tap is negative or not finite"; return false; }
            out.p.psf_size = size;
        }
        else if (key == "seed") {
            char* end = nullptr;
            out.p.seed = std::strtoull(v.c_str(), &end, 0);
            if (v.empty() || *end || v[0] == '-') { why = "seed needs an unsigned integer, not '" + v + "'"; return false; }
        }
        else if (!number(key, v, x)) return false;
        else if (key == "gain") out.p.gain_e = (float)x;
        else if (key == "read") out.p.read_e = (float)x;
        else if (key == "dark") out.p.dark_e = (float)x;
        else if (key == "prnu") out.p.prnu = (float)x;
        else if (key == "dsnu") out.p.dsnu_e = (float)x;
        else if (key == "well") out.p.full_well_e = (float)x;
        else if (key == "epdn") out.p.e_per_dn = (float)x;
        else if (key == "offset") out.p.offset_dn = (float)x;
        else if (key == "bits" || key == "mono" || key == "noise") {
            if (x != std::floor(x) || std::fabs(x) > 64.0) { why = key + " needs a small integer"; return false; }
            (key == "bits" ? out.p.bits : key == "mono" ? out.p.mono : out.p.noise) = (int)x;
        }
        else { why = "unknown key '" + key + "'; known keys: psf gain read dark prnu dsnu well epdn offset bits mono noise seed"; return false; }
    }
    const DsrtSensor& p = out.p;
    if (!(p.gain_e > 0.0f) || !(p.e_per_dn > 0.0f) || !(p.full_well_e > 0.0f)) { why = "gain, epdn and well must be > 0"; return false; }
    if (!(p.prnu >= 0.0f) || !(p.dark_e >= 0.0f) || !(p.dsnu_e >= 0.0f) || !(p.read_e >= 0.0f)) { why = "prnu, dark, dsnu and read must be >= 0"; return false; }
    if (!std::isfinite(p.offset_dn)) { why = "offset must be finite"; return false; }
    if (p.bits < 8 || p.bits > 16) { why = "bits must be between 8 and 16"; return false; }
    if ((p.mono != 0 && p.mono != 1) || (p.noise != 0 && p.noise != 1)) { why = "mono and noise are 0 or 1"; return false; }
    return true;
}

static int fail(const char* what) {
    std::fprintf(stderr, "dsrt_render: %s: %s\n", what, dsrt_last_error());
    return 1;
}

int main(int argc, char** argv) {
    std::string pose_file, out_dir = "output", obj;
    int width = 800, height = 450, spp = 1000, depth = 50, first = 0, count = -1, rng_mode = 0, math_mode = 0, passes = 0;
    int adaptive_passes = 8, adaptive_min = 2;
    float adaptive_tol = 0.0f, adaptive_floor = 0.0f;
    bool adaptive = false, adaptive_detail = false, denoise = false, temporal = false, flow = false, follow_bodies = false, follow_shading = false;
    int denoise_iterations = -1;                                    // -1: the library's default
    bool coverage = false, coverage_aware = false;
    DsrtCoverageDesc cov_desc{DSRT_COVERAGE_DIAGONAL, 64};
    float alpha_min = dsrt_denoise_coverage_alpha_min();            // (with --upscale: dsrt_upscale_coverage_alpha_min(), unless a value is given)
    bool alpha_min_given = false;
    const char* usage_coverage = "dsrt_render: --coverage takes grid:S (S = 1 .. 8) or diag:N (N = 1 .. 64)\n";
    bool upscale = false;
    int upscale_factor = 4;                                         // the reference's scale (src/main.cpp:444)
    std::vector<std::pair<std::string, double>> bodies;             // --body OBJ [--body-scale S], repeatable: movable rigid bodies 1, 2, ... (include/dsrt.h, MOVABLE RIGID BODIES)
    std::string body_poses_file;                                    // --body-poses FILE: one line per rendered frame, 12 numbers per body (row-major 3x4 [R | t], model frame)
    bool sah = false, lbvh = false, png = false, strict_textures = false, certified = false, gbuffer = false, variance = false;
    bool sensor = false;
    SensorSpec sensor_spec;                                         // --sensor SPEC (include/dsrt.h, SENSOR MODEL)
    bool stars = false;
    StarsSpec stars_spec;                                           // --stars FILE[,flux=F][,occlusion=0] (include/dsrt.h, POINT SOURCES)
    bool lens = false;
    LensSpec lens_spec;                                             // --lens SPEC (include/dsrt.h, LENS MODEL)
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        auto next = [&](const char* flag) -> const char* {
            if (i + 1 >= argc) { std::fprintf(stderr, "dsrt_render: %s needs a value\n", flag); std::exit(2); }
            return argv[++i];
        };
        if (a == "--input_txt") pose_file = next("--input_txt");
        else if (a == "--output_dir") out_dir = next("--output_dir");
        else if (a == "--obj") obj = next("--obj");
        else if (a == "--width") width = std::atoi(next("--width"));
        else if (a == "--height") height = std::atoi(next("--height"));
        else if (a == "--spp") spp = std::atoi(next("--spp"));
        else if (a == "--depth") depth = std::atoi(next("--depth"));
        else if (a == "--frame") first = std::atoi(next("--frame"));
        else if (a == "--frames") count = std::atoi(next("--frames"));
        else if (a == "--fast") { sah = true; rng_mode = 1; }      // non-parity fast mode: SAH tree + Philox stream per sample (include/dsrt.h)
        else if (a == "--bvh") { const std::string k = next("--bvh"); sah = k == "sah"; lbvh = k == "lbvh"; }      // lbvh: built on the GPU (milliseconds), non-parity like sah
        else if (a == "--rng-mode") rng_mode = std::atoi(next("--rng-mode"));
        else if (a == "--reference-math") math_mode = 1;          // sinf / cosf / powf from the device math library: the reference's own kernel's bytes on this GPU (include/dsrt.h)
        else if (a == "--certified-tree") certified = true;        // rays walk the certified second tree: the reference's bytes, a third fewer node visits (include/dsrt.h)
        else if (a == "--strict-textures") strict_textures = true;  // refuse a mesh whose texture maps this library cannot decode (include/dsrt.h)
        else if (a == "--gbuffer") gbuffer = true;                  // ground-truth channels of every frame next to its image (include/dsrt.h, dsrt_render_gbuffer)
        else if (a == "--png") png = true;                          // frames as PNG instead of PPM (the reference converts with ImageMagick)
        else if (a == "--passes") passes = std::atoi(next("--passes"));   // rng_mode 1: each frame as P interleaved sample sets, an image after each (include/dsrt.h, SAMPLE SETS)
        else if (a == "--variance") variance = true;                // rng_mode 1: also the variance of each pixel's mean, <frame>_var.pfm
        else if (a == "--adaptive") { adaptive = true; adaptive_tol = (float)std::atof(next("--adaptive")); }   // rng_mode 1: adaptive sampling to this relative standard error
        else if (a == "--adaptive-passes") { adaptive_detail = true; adaptive_passes = std::atoi(next("--adaptive-passes")); }
        else if (a == "--adaptive-min-passes") { adaptive_detail = true; adaptive_min = std::atoi(next("--adaptive-min-passes")); }
        else if (a == "--adaptive-floor") { adaptive_detail = true; adaptive_floor = (float)std::atof(next("--adaptive-floor")); }
        else if (a == "--denoise") {                                // rng_mode 1: the variance-guided filter over each frame; the value (iterations) is optional
            denoise = true;
            if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') denoise_iterations = std::atoi(argv[++i]);
        }
        else if (a == "--coverage") {                               // sub-pixel coverage of every frame next to its image (include/dsrt.h, COVERAGE)
            const std::string v = next("--coverage");
            coverage = true;
            if (v.rfind("grid:", 0) == 0) cov_desc.pattern = DSRT_COVERAGE_GRID;
            else if (v.rfind("diag:", 0) == 0) cov_desc.pattern = DSRT_COVERAGE_DIAGONAL;
            else { std::fputs(usage_coverage, stderr); return 2; }
            char* end = nullptr;
            const long k = std::strtol(v.c_str() + 5, &end, 10);
            if (end == v.c_str() + 5 || *end || k < 1 || k > (cov_desc.pattern == DSRT_COVERAGE_GRID ? 8 : 64)) { std::fputs(usage_coverage, stderr); return 2; }
            cov_desc.samples = (int)k;
        }
        else if (a == "--coverage-aware") {                         // with --denoise: the filter works on the covered part of every pixel; the value (alpha_min) is optional
            coverage_aware = true;
            if (i + 1 < argc && ((argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') || argv[i + 1][0] == '.')) { alpha_min = (float)std::atof(argv[++i]); alpha_min_given = true; }
        }
        else if (a == "--temporal") temporal = true;                // with --denoise: reprojected frame history (include/dsrt.h, TEMPORAL ACCUMULATION)
        else if (a == "--flow") flow = true;                        // with --temporal: <frame>_flow.pfm, every pixel's displacement from the previous frame
        else if (a == "--follow-bodies") follow_bodies = true;      // with --body, --denoise and --temporal: the history follows the bodies (include/dsrt.h, TEMPORAL ACCUMULATION WITH BODIES)
        else if (a == "--follow-shading") follow_shading = true;    // with --denoise and --temporal: the history follows the sun state (include/dsrt.h, TEMPORAL ACCUMULATION THAT FOLLOWS SHADING)
        else if (a == "--body") bodies.emplace_back(next("--body"), 1.0);
        else if (a == "--body-scale") {
            const double sc = std::atof(next("--body-scale"));
            if (bodies.empty()) { std::fprintf(stderr, "dsrt_render: --body-scale follows the --body it scales\n"); return 2; }
            bodies.back().second = sc;
        }
        else if (a == "--body-poses") body_poses_file = next("--body-poses");
        else if (a == "--upscale") {                                // rng_mode 1: G-buffer-guided upscaling by the optional factor (include/dsrt.h, UPSCALER)
            upscale = true;
            if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') upscale_factor = std::atoi(argv[++i]);
        }
        else if (a == "--sensor") {                                 // rng_mode 1: the detector model over each frame's linear image (include/dsrt.h, SENSOR MODEL)
            std::string why;
            if (!parse_sensor_spec(next("--sensor"), sensor_spec, why)) { std::fprintf(stderr, "dsrt_render: --sensor: %s\n", why.c_str()); return 2; }
            sensor = true;
        }
        else if (a == "--stars") {                                  // rng_mode 1: a star field added to each frame's linear image (include/dsrt.h, POINT SOURCES)
            std::string why;
            if (!parse_stars_spec(next("--stars"), stars_spec, why)) { std::fprintf(stderr, "dsrt_render: --stars: %s\n", why.c_str()); return 2; }
            stars = true;
        }
        else if (a == "--lens") {                                   // rng_mode 1: distortion and vignetting on each frame's linear image (include/dsrt.h, LENS MODEL)
            std::string why;
            if (!parse_lens_spec(next("--lens"), lens_spec, why)) { std::fprintf(stderr, "dsrt_render: --lens: %s\n", why.c_str()); return 2; }
            lens = true;
        }
        else { std::fprintf(stderr, "usage: dsrt_render --obj mesh.obj [--input_txt poses.txt] [--output_dir dir] [--width W --height H --spp N --depth D] [--frame i --frames n] [--bvh median|sah|lbvh] [--rng-mode 0|1] [--reference-math] [--certified-tree] [--fast] [--png] [--gbuffer] [--strict-textures] [--passes P] [--variance] [--adaptive TOL [--adaptive-passes P] [--adaptive-min-passes M] [--adaptive-floor F]] [--denoise [ITER]] [--temporal] [--flow] [--upscale [S]] [--body body.obj [--body-scale S]]... [--body-poses poses.txt] [--follow-bodies] [--follow-shading] [--coverage grid:S|diag:N] [--coverage-aware [ALPHA_MIN]] [--rng-mode 1 --upscale [S] --coverage-aware [ALPHA_MIN] [--coverage diag:N]] [--rng-mode 1 --sensor SPEC] [--rng-mode 1 --stars FILE[,flux=F][,occlusion=0]] [--rng-mode 1 --lens SPEC]\n"); return 2; }
    }
    if (obj.empty()) { std::fprintf(stderr, "dsrt_render: --obj is required\n"); return 2; }
    if (!bodies.empty() && (sah || lbvh || certified)) { std::fprintf(stderr, "dsrt_render: --body brings its own tree: it does not combine with --bvh sah|lbvh, --fast or --certified-tree\n"); return 2; }
    if ((int)bodies.size() > DSRT_MAX_BODIES - 1) { std::fprintf(stderr, "dsrt_render: at most %d --body\n", DSRT_MAX_BODIES - 1); return 2; }
    if (!body_poses_file.empty() && bodies.empty()) { std::fprintf(stderr, "dsrt_render: --body-poses needs --body\n"); return 2; }
    if (upscale && coverage_aware && rng_mode != 1) { std::fprintf(stderr, "dsrt_render: --upscale --coverage-aware needs --rng-mode 1 (or --fast)\n"); return 2; }
    if (upscale && coverage_aware && coverage && cov_desc.pattern != DSRT_COVERAGE_DIAGONAL) { std::fprintf(stderr, "dsrt_render: --upscale --coverage-aware takes --coverage diag:N (N = 1 .. 64), not a grid: pattern\n"); return 2; }
    if (upscale && rng_mode != 1) {                                 // the reference's bytes are not upscaled here: the flag is announced and ignored, as it always was
        std::fprintf(stderr, "dsrt_render: --upscale is not supported (post-process outside this library)\n");
        upscale = false;
    }
    if (sensor && rng_mode != 1) {                                  // the linear frame is rng_mode 1's: announced and ignored, like --upscale
        std::fprintf(stderr, "dsrt_render: --sensor needs --rng-mode 1 (or --fast): ignored\n");
        sensor = false;
    }
    if (stars && rng_mode != 1) {                                   // announced and ignored, like --sensor
        std::fprintf(stderr, "dsrt_render: --stars needs --rng-mode 1 (or --fast): ignored\n");
        stars = false;
    }
    if (lens && rng_mode != 1) {                                    // announced and ignored, like --sensor
        std::fprintf(stderr, "dsrt_render: --lens needs --rng-mode 1 (or --fast): ignored\n");
        lens = false;
    }
    if (lens && (adaptive || passes != 0 || gbuffer)) { std::fprintf(stderr, "dsrt_render: --lens does not combine with --adaptive / --passes / --gbuffer\n"); return 2; }
    if (lens && spp < 2) { std::fprintf(stderr, "dsrt_render: --lens needs --spp 2 or more\n"); return 2; }
    if (stars && (adaptive || passes != 0 || gbuffer)) { std::fprintf(stderr, "dsrt_render: --stars does not combine with --adaptive / --passes / --gbuffer\n"); return 2; }
    if (stars && spp < 2) { std::fprintf(stderr, "dsrt_render: --stars needs --spp 2 or more\n"); return 2; }
    if (sensor && (adaptive || passes != 0 || gbuffer)) { std::fprintf(stderr, "dsrt_render: --sensor does not combine with --adaptive / --passes / --gbuffer\n"); return 2; }
    if (sensor && spp < 2) { std::fprintf(stderr, "dsrt_render: --sensor needs --spp 2 or more\n"); return 2; }
    if (upscale && (upscale_factor < 2 || upscale_factor > 8)) { std::fprintf(stderr, "dsrt_render: --upscale S must be between 2 and 8\n"); return 2; }
    if (upscale && (temporal || adaptive || passes != 0 || gbuffer)) { std::fprintf(stderr, "dsrt_render: --upscale does not combine with --temporal / --adaptive / --passes / --gbuffer\n"); return 2; }
    if (upscale && spp < 2) { std::fprintf(stderr, "dsrt_render: --upscale needs --spp 2 or more\n"); return 2; }
    if (adaptive_detail && !adaptive) { std::fprintf(stderr, "dsrt_render: --adaptive-passes, --adaptive-min-passes and --adaptive-floor need --adaptive TOL\n"); return 2; }
    if (adaptive && rng_mode != 1) { std::fprintf(stderr, "dsrt_render: --adaptive needs --rng-mode 1 (or --fast)\n"); return 2; }
    if (adaptive && (passes != 0 || gbuffer)) { std::fprintf(stderr, "dsrt_render: --adaptive does not combine with --passes / --gbuffer\n"); return 2; }
    if (adaptive && !(adaptive_tol >= 0.0f && adaptive_floor >= 0.0f)) { std::fprintf(stderr, "dsrt_render: --adaptive and --adaptive-floor must be >= 0\n"); return 2; }
    if (adaptive && (adaptive_passes < 1 || adaptive_passes > std::min(std::max(spp, 1), 64))) { std::fprintf(stderr, "dsrt_render: --adaptive-passes must be between 1 and min(--spp, 64)\n"); return 2; }
    if (adaptive && (adaptive_min < 1 || adaptive_min > adaptive_passes)) { std::fprintf(stderr, "dsrt_render: --adaptive-min-passes must be between 1 and --adaptive-passes\n"); return 2; }
    if (denoise && rng_mode != 1) { std::fprintf(stderr, "dsrt_render: --denoise needs --rng-mode 1 (or --fast)\n"); return 2; }
    if (denoise && (passes != 0 || adaptive || gbuffer)) { std::fprintf(stderr, "dsrt_render: --denoise does not combine with --passes / --adaptive / --gbuffer\n"); return 2; }
    if (denoise && denoise_iterations > 6) { std::fprintf(stderr, "dsrt_render: --denoise ITER must be between 0 and 6\n"); return 2; }
    if (denoise && spp < 2) { std::fprintf(stderr, "dsrt_render: --denoise needs --spp 2 or more\n"); return 2; }
    if (coverage_aware && !denoise && !upscale) { std::fprintf(stderr, "dsrt_render: --coverage-aware needs --denoise or --upscale\n"); return 2; }
    if (coverage_aware && (temporal || (denoise && upscale))) { std::fprintf(stderr, "dsrt_render: --coverage-aware does not combine with --temporal, nor with --denoise and --upscale together\n"); return 2; }
    if (coverage_aware && !(alpha_min > 0.0f && alpha_min <= 1.0f)) { std::fprintf(stderr, "dsrt_render: --coverage-aware ALPHA_MIN must be > 0 and <= 1\n"); return 2; }
    if (temporal && !denoise) { std::fprintf(stderr, "dsrt_render: --temporal needs --denoise\n"); return 2; }
    if (flow && !temporal) { std::fprintf(stderr, "dsrt_render: --flow needs --temporal\n"); return 2; }
    if (follow_shading && (!denoise || !temporal)) { std::fprintf(stderr, "dsrt_render: --follow-shading needs --denoise and --temporal\n"); return 2; }
    if (follow_bodies && (bodies.empty() || !denoise || !temporal)) { std::fprintf(stderr, "dsrt_render: --follow-bodies needs --body, --denoise and --temporal\n"); return 2; }
    if ((passes != 0 || variance) && rng_mode != 1) { std::fprintf(stderr, "dsrt_render: --passes and --variance need --rng-mode 1 (or --fast)\n"); return 2; }
    if (passes < 0 || passes > std::max(spp, 1)) { std::fprintf(stderr, "dsrt_render: --passes must be between 1 and --spp\n"); return 2; }
    if (variance && spp < 2) { std::fprintf(stderr, "dsrt_render: --variance needs --spp 2 or more\n"); return 2; }
    if ((passes != 0 || variance) && gbuffer) { std::fprintf(stderr, "dsrt_render: --gbuffer does not combine with --passes / --variance\n"); return 2; }
    mkdir(out_dir.c_str(), 0777);

    std::vector<DsrtPose> poses;
    if (!pose_file.empty()) {
        int n = 0;
        if (dsrt_read_pose_file(pose_file.c_str(), nullptr, 0, &n) == DSRT_OK) {
            poses.resize((size_t)n);
            dsrt_read_pose_file(pose_file.c_str(), poses.data(), n, &n);
        }
    }
    if (poses.empty()) {                                   // the reference's default pose, src/main.cpp:275-284
        std::printf("No valid pose file found; using single default pose.\n");
        DsrtPose p{};
        p.cam_pos_world[0] = 0.0; p.cam_pos_world[1] = 50.0; p.cam_pos_world[2] = 200.0;
        p.model_pos_world[0] = 0.0; p.model_pos_world[1] = -100.0; p.model_pos_world[2] = 0.0;
        poses.push_back(p);
    } else {
        std::printf("Loaded %zu poses.\n", poses.size());
    }

    DsrtHostScene* hs = dsrt_host_scene_create();
    if (dsrt_host_scene_add_obj(hs, obj.c_str(), 1.0) != DSRT_OK) return fail("loading the mesh");
    {
        char names[4096];
        const int bad = dsrt_host_scene_texture_failures(hs, names, sizeof names);
        if (bad) {
            std::fprintf(stderr, "dsrt_render: %d texture map(s) could not be decoded (GIF, PSD, PIC, HDR and CMYK JPEG are not read here; the reference's stb_image reads them);\n"
                                 "they render as the reference's 1x1 white fallback, i.e. NOT like the reference would:\n%s", bad, names);
            if (strict_textures) return 3;
        }
    }
    for (const auto& b : bodies) {
        if (dsrt_host_scene_begin_body(hs) < 0) return fail("starting a body");
        if (dsrt_host_scene_add_obj(hs, b.first.c_str(), b.second) != DSRT_OK) return fail("loading a body's mesh");
    }
    // one line of 12 numbers per body for every RENDERED frame, in order; frames past the last line keep the last poses
    std::vector<std::vector<float>> body_poses;
    if (!body_poses_file.empty()) {
        std::ifstream in(body_poses_file);
        if (!in) { std::fprintf(stderr, "dsrt_render: cannot open %s\n", body_poses_file.c_str()); return 1; }
        std::string line;
        while (std::getline(in, line)) {
            if (line.empty() || line[0] == '#') continue;
            std::istringstream is(line);
            std::vector<float> v;
            for (double x; is >> x;) v.push_back((float)x);
            if (v.size() != 12 * bodies.size()) { std::fprintf(stderr, "dsrt_render: %s: a line needs 12 numbers for each of the %zu bodies\n", body_poses_file.c_str(), bodies.size()); return 2; }
            body_poses.push_back(v);
        }
    }
    if (!bodies.empty()) {
        if (dsrt_host_scene_build_bvh_bodies(hs) != DSRT_OK) return fail("building the bodies tree");
    } else {
        float build_ms = 0.0f, total_ms = 0.0f;
        const int rc = lbvh ? dsrt_host_scene_build_bvh_gpu(hs, 0, &build_ms, &total_ms) : (sah ? dsrt_host_scene_build_bvh_sah(hs) : dsrt_host_scene_build_bvh(hs));
        if (rc != DSRT_OK) return fail("building the BVH");
        if (lbvh) std::printf("BVH built on the GPU: %.2f ms of kernels, %.2f ms with upload and copy-back\n", build_ms, total_ms);
    }
    GPUScene scene;
    if (dsrt_host_scene_view(hs, &scene) != DSRT_OK) return fail("viewing the scene");
    std::printf("mesh: %d triangles, %d BVH nodes, %d materials\n", scene.num_triangles, scene.num_bvh_nodes, scene.num_materials);

    DsrtContext* ctx = nullptr;
    if (dsrt_ctx_create(0, &ctx) != DSRT_OK) return fail("creating the device context");
    if (follow_bodies && dsrt_ctx_set_temporal_bodies(ctx, 1) != DSRT_OK) return fail("setting the context to follow the bodies");
    if (follow_shading && dsrt_ctx_set_temporal_shading(ctx, 2) != DSRT_OK) return fail("setting the context to follow the shading");
    if (certified && dsrt_ctx_set_certified_tree(ctx, 1) != DSRT_OK) return fail("asking for the certified second tree");
    // The reference's loop renders frame after frame (src/main.cpp:310-431).  Here the poses of a run are rendered as batch launches
    // (dsrt_render_batch_to_host: up to 32 frames as ONE pool of work, include/dsrt.h) and written out in pose order afterwards: each
    // frame's image is byte for byte what a launch of its own would give, the run is simply not held up by every frame's tail.
    const size_t last = count < 0 ? poses.size() : std::min(poses.size(), (size_t)(first + count));
    std::vector<size_t> ids;
    std::vector<GPUCamera> cams;
    std::vector<float> suns;
    for (size_t i = (size_t)first; i < last; ++i) {
        DsrtFrame fr;
        dsrt_pose_to_frame(&poses[i], &fr);
        std::printf("\n=== Frame %zu ===\n  sep(cam, model) = %g m\n", i, fr.sep_m);
        if (fr.skipped) { std::printf("  [!] Camera is inside/too close to ISS mesh. Skipping frame.\n"); continue; }
        GPUCamera cam;
        const float origin[3] = {0.0f, 0.0f, 0.0f};
        if (dsrt_camera_look_at(&cam, fr.cam_in_model, origin, 40.0f, width, height, spp, depth) != DSRT_OK) return fail("camera");
        if (ids.empty()) {
            dsrt_scene_set_frame(&scene, &cam, fr.sun_dir_model);
            if ((bodies.empty() ? dsrt_scene_upload(ctx, &scene) : dsrt_scene_upload_bodies(ctx, hs, &scene)) != DSRT_OK) return fail("uploading the scene");
        }
        ids.push_back(i); cams.push_back(cam);
        suns.insert(suns.end(), fr.sun_dir_model, fr.sun_dir_model + 3);
    }
    DsrtRenderDesc d;
    std::memset(&d, 0, sizeof d);
    d.width = width; d.height = height; d.spp = spp; d.max_depth = depth; d.gamma = 2.0f; d.seed = 1337; d.rng_mode = rng_mode; d.math_mode = math_mode;
    const size_t px = (size_t)width * height, image_bytes = px * 3;
    const std::string ext = png ? ".png" : ".ppm";
    auto frame_base = [&](size_t id) { char stem[64]; std::snprintf(stem, sizeof stem, "/frame_%04zu", id); return out_dir + stem; };
    auto write_image = [&](const std::string& path, const uint8_t* image) {
        return (png ? dsrt_write_png(path.c_str(), image, width, height) : dsrt_write_ppm(path.c_str(), image, width, height)) == DSRT_OK;
    };

    // --sensor, --stars, --lens: every chain below also hands out its LINEAR image (at the upscaler's output size with --upscale), the star field's and the detector's input.
    const bool wants_linear = sensor || stars || lens;
    const int sensor_w = upscale ? width * upscale_factor : width, sensor_h = upscale ? height * upscale_factor : height;
    std::vector<float> sensor_linear(wants_linear ? (size_t)sensor_w * sensor_h * 3 : 0);
    float* const lin = wants_linear ? sensor_linear.data() : nullptr;
    const std::string undenoised = sensor ? "_noisy" : "_raw";     // (with --sensor, _raw is the detector's raw frame)

    // The modes that render frame by frame: one step each, over buffers that stay empty where the mode does not use them.
    const bool host_sums = !upscale && ((denoise && !temporal) || (!denoise && !adaptive && (passes != 0 || variance)));
    std::vector<uint8_t> img(image_bytes), raw(denoise && !upscale ? image_bytes : 0);
    std::vector<float> var(variance && !upscale ? image_bytes : 0);
    std::vector<uint64_t> sum(host_sums ? image_bytes : 0), sq(host_sums && (denoise || variance) ? image_bytes : 0);
    const DsrtAccum acc{sum.data(), sq.empty() ? nullptr : sq.data()};
    auto write_var = [&](const std::string& base) { return !variance || dsrt_write_pfm((base + "_var.pfm").c_str(), var.data(), width, height, 3) == DSRT_OK; };
    DsrtDenoise dn;
    dsrt_denoise_defaults(&dn);
    if (denoise_iterations >= 0) dn.iterations = denoise_iterations;
    std::function<int(size_t, const std::string&)> frame_step;           // (index into ids, <out_dir>/frame_NNNN) -> exit code; empty: the batch launches below

    std::vector<uint32_t> n(adaptive ? px : 0);
    std::vector<float> spp_map(adaptive ? px : 0);
    const DsrtAdaptive ad{adaptive_passes, adaptive_min, adaptive_tol, adaptive_floor};
    if (adaptive) frame_step = [&](size_t, const std::string& base) -> int {
        DsrtAdaptiveStats st;
        if (dsrt_render_adaptive_to_host(ctx, &d, &ad, n.data(), img.data(), nullptr, variance ? var.data() : nullptr, &st) != DSRT_OK) return fail("rendering adaptively");
        const std::string path = base + ext;
        if (!write_image(path, img.data())) return fail("writing the frame");
        for (size_t i = 0; i < px; ++i) spp_map[i] = (float)n[i];
        if (dsrt_write_pfm((base + "_spp.pfm").c_str(), spp_map.data(), width, height, 1) != DSRT_OK) return fail("writing the sample counts");
        if (!write_var(base)) return fail("writing the variance");
        std::printf("adaptive: %d of %d passes, %.1f %% of the frame's %d samples per pixel; pixels per pass:", st.passes_run, adaptive_passes,
                    100.0 * (double)st.samples_total / ((double)px * spp), spp);
        for (int p = 0; p < st.passes_run; ++p) std::printf(" %u", st.active[p]);
        std::printf("\nSaved %s, %s_spp.pfm%s\n", path.c_str(), base.c_str(), variance ? " and _var.pfm" : "");
        return 0;
    };

    // --denoise --temporal: each frame in pose order through the convenience form, the history kept by the context; the raw image is the same samples in one launch.
    std::vector<float> prev_xy(flow ? px * 2 : 0), flow_px(flow ? px * 3 : 0);
    DsrtTemporal tp;
    dsrt_temporal_defaults(&tp);
    if (denoise && temporal) frame_step = [&](size_t q, const std::string& base) -> int {
        d.seed = 1337 + (uint64_t)ids[q];
        if (dsrt_render_denoised_temporal_to_host(ctx, &d, &dn, &tp, q == 0 ? 1 : 0, img.data(), nullptr, lin, variance ? var.data() : nullptr,
                                                  flow ? prev_xy.data() : nullptr, nullptr) != DSRT_OK) return fail("rendering with temporal accumulation");
        if (dsrt_render_to_host(ctx, &d, raw.data(), nullptr, nullptr) != DSRT_OK) return fail("rendering the raw image");
        if (!write_image(base + ext, img.data()) || !write_image(base + undenoised + ext, raw.data())) return fail("writing the frame");
        if (!write_var(base)) return fail("writing the variance");
        if (flow) {
            for (size_t i = 0; i < px; ++i) {
                flow_px[3 * i + 0] = prev_xy[2 * i + 0] - (float)(i % (size_t)width);
                flow_px[3 * i + 1] = prev_xy[2 * i + 1] - (float)(i / (size_t)width);
                flow_px[3 * i + 2] = 0.0f;
            }
            if (dsrt_write_pfm((base + "_flow.pfm").c_str(), flow_px.data(), width, height, 3) != DSRT_OK) return fail("writing the flow");
        }
        std::printf("denoise: %d iterations, temporal, seed %llu\nSaved %s, %s%s%s%s%s\n", dn.iterations, (unsigned long long)d.seed, (base + ext).c_str(), base.c_str(),
                    undenoised.c_str(), ext.c_str(), variance ? ", _var.pfm" : "", flow ? ", _flow.pfm" : "");
        return 0;
    };

    // --denoise: each frame's sums with second moments, the raw image they resolve to, the G-buffer of its camera, the filter (include/dsrt.h, DENOISER).
    const bool guided = denoise && !temporal && !upscale;
    std::vector<float> normal(guided ? image_bytes : 0), position(guided ? image_bytes : 0), albedo(guided ? image_bytes : 0), range(guided ? px : 0);
    const DsrtDenoiseGuides guides{normal.data(), position.data(), albedo.data(), range.data()};
    std::vector<float> alpha(guided && coverage_aware ? px : 0);
    DsrtGBuffer g;
    std::memset(&g, 0, sizeof g);
    g.normal = normal.data(); g.position = position.data(); g.albedo = albedo.data(); g.range = range.data();
    if (guided) frame_step = [&](size_t, const std::string& base) -> int {
        std::fill(sum.begin(), sum.end(), 0);
        std::fill(sq.begin(), sq.end(), 0);
        if (dsrt_render_accumulate_to_host(ctx, &d, 0, spp, 1, &acc, nullptr) != DSRT_OK) return fail("rendering the samples");
        if (dsrt_resolve_accumulated_to_host(ctx, &d, &acc, spp, raw.data(), nullptr, nullptr) != DSRT_OK) return fail("resolving the raw image");
        if (coverage_aware) {                                       // alpha and the representatives' guides from a DIAGONAL 64 pass: the renderer's own measure
            DsrtCoverageDesc cd;
            dsrt_coverage_defaults(&cd);
            DsrtCoverage cv;
            std::memset(&cv, 0, sizeof cv);
            cv.alpha = alpha.data(); cv.rep = g;
            if (dsrt_render_coverage_to_host(ctx, &d, &cd, nullptr, &cv, nullptr) != DSRT_OK) return fail("rendering the coverage");
            if (dsrt_denoise_accumulated_coverage_to_host(ctx, &d, &acc, spp, nullptr, &guides, alpha.data(), alpha_min, &dn, img.data(), nullptr, lin,
                                                          variance ? var.data() : nullptr) != DSRT_OK) return fail("denoising");
        } else {
        if (dsrt_render_gbuffer_to_host(ctx, &d, &g, nullptr) != DSRT_OK) return fail("rendering the G-buffer");
        if (dsrt_denoise_accumulated_to_host(ctx, &d, &acc, spp, nullptr, &guides, &dn, img.data(), nullptr, lin, variance ? var.data() : nullptr) != DSRT_OK)
            return fail("denoising");
        }
        if (!write_image(base + ext, img.data()) || !write_image(base + undenoised + ext, raw.data())) return fail("writing the frame");
        if (!write_var(base)) return fail("writing the variance");
        if (coverage_aware) std::printf("coverage-aware: alpha_min %g\n", (double)alpha_min);
        std::printf("denoise: %d iterations\nSaved %s, %s%s%s%s\n", dn.iterations, (base + ext).c_str(), base.c_str(), undenoised.c_str(), ext.c_str(), variance ? " and _var.pfm" : "");
        return 0;
    };

    // --passes / --variance: each frame as P interleaved sample sets (first = p, stride = P) added into one pair of sums: after pass p every pixel holds samples from
    // its whole area, and after the last the image is the one-launch image byte for byte (include/dsrt.h, SAMPLE SETS).
    if (!adaptive && !denoise && !upscale && !wants_linear && (passes != 0 || variance)) frame_step = [&](size_t, const std::string& base) -> int {
        const int P = passes > 0 ? passes : 1;
        std::fill(sum.begin(), sum.end(), 0ull);
        std::fill(sq.begin(), sq.end(), 0ull);
        int done = 0;
        for (int p = 0; p < P; ++p) {
            const int count = (spp - p + P - 1) / P;
            DsrtStats st;
            if (dsrt_render_accumulate_to_host(ctx, &d, p, count, P, &acc, &st) != DSRT_OK) return fail("rendering a pass");
            done += count;
            if (dsrt_resolve_accumulated_to_host(ctx, &d, &acc, done, img.data(), nullptr, nullptr) != DSRT_OK) return fail("resolving a pass");
            const std::string path = p + 1 < P || passes > 0 ? base + "_pass" + std::to_string(p + 1) + "of" + std::to_string(P) + ext : base + ext;
            if (!write_image(path, img.data())) return fail("writing the frame");
            std::printf("pass %d/%d: %d samples per pixel, kernel %.3f ms; saved %s\n", p + 1, P, done, st.kernel_ms, path.c_str());
        }
        if (passes > 0 && !write_image(base + ext, img.data())) return fail("writing the frame");
        if (variance) {
            if (dsrt_resolve_accumulated_to_host(ctx, &d, &acc, done, nullptr, nullptr, var.data()) != DSRT_OK) return fail("resolving the variance");
            if (!write_var(base)) return fail("writing the variance");
            std::printf("Saved %s_var.pfm\n", base.c_str());
        }
        std::printf("Saved %s%s\n", base.c_str(), ext.c_str());
        return 0;
    };

    // --upscale: the frame at --width x --height (denoised with --denoise), both rasters' G-buffers and the guided upscaler, through the convenience form.
    const int out_w = width * upscale_factor, out_h = height * upscale_factor;
    const size_t out_values = upscale ? (size_t)out_w * out_h * 3 : 0;
    std::vector<uint8_t> big(out_values);
    std::vector<float> big_var(variance ? out_values : 0);
    DsrtUpscale up;
    dsrt_upscale_defaults(&up);
    const bool upscale_coverage = upscale && coverage_aware;        // (--coverage then only chooses the passes' N: it writes no files of its own)
    DsrtCoverageDesc up_cov;
    dsrt_coverage_defaults(&up_cov);
    if (upscale_coverage && coverage) { up_cov = cov_desc; coverage = false; }
    if (upscale_coverage && !alpha_min_given) alpha_min = dsrt_upscale_coverage_alpha_min();
    std::vector<float> big_alpha(upscale_coverage ? (size_t)out_w * out_h : 0);
    if (upscale_coverage) frame_step = [&](size_t, const std::string& base) -> int {
        if (dsrt_render_upscaled_coverage_to_host(ctx, &d, out_w, out_h, &up_cov, &up_cov, alpha_min, nullptr, &up, big.data(), nullptr, lin,
                                                  variance ? big_var.data() : nullptr, img.data(), big_alpha.data(), nullptr) != DSRT_OK) return fail("rendering and upscaling with coverage");
        const std::string path = base + ext;
        if ((png ? dsrt_write_png(path.c_str(), big.data(), out_w, out_h) : dsrt_write_ppm(path.c_str(), big.data(), out_w, out_h)) != DSRT_OK ||
            !write_image(base + "_lowres" + ext, img.data())) return fail("writing the frame");
        if (dsrt_write_pfm((base + "_alpha.pfm").c_str(), big_alpha.data(), out_w, out_h, 1) != DSRT_OK) return fail("writing the alpha");
        if (variance && dsrt_write_pfm((base + "_var.pfm").c_str(), big_var.data(), out_w, out_h, 3) != DSRT_OK) return fail("writing the variance");
        std::printf("upscale: %d x %d -> %d x %d, coverage-aware: DIAGONAL %d, alpha_min %g\nSaved %s, %s_lowres%s, _alpha.pfm%s\n", width, height, out_w, out_h, up_cov.samples,
                    (double)alpha_min, path.c_str(), base.c_str(), ext.c_str(), variance ? " and _var.pfm" : "");
        return 0;
    };
    else if (upscale) frame_step = [&](size_t, const std::string& base) -> int {
        if (dsrt_render_upscaled_to_host(ctx, &d, out_w, out_h, denoise ? &dn : nullptr, &up, big.data(), nullptr, lin, variance ? big_var.data() : nullptr, img.data(),
                                         nullptr) != DSRT_OK) return fail("rendering and upscaling");
        const std::string path = base + ext;
        if ((png ? dsrt_write_png(path.c_str(), big.data(), out_w, out_h) : dsrt_write_ppm(path.c_str(), big.data(), out_w, out_h)) != DSRT_OK ||
            !write_image(base + "_lowres" + ext, img.data())) return fail("writing the frame");
        if (variance && dsrt_write_pfm((base + "_var.pfm").c_str(), big_var.data(), out_w, out_h, 3) != DSRT_OK) return fail("writing the variance");
        std::printf("upscale: %d x %d -> %d x %d%s\nSaved %s, %s_lowres%s%s\n", width, height, out_w, out_h, denoise ? ", denoised in between" : "", path.c_str(), base.c_str(),
                    ext.c_str(), variance ? " and _var.pfm" : "");
        return 0;
    };

    // --gbuffer: the ground truth of the frame the context's camera, sun and body poses are set to
    auto write_gbuffer = [&](const std::string& base) -> int {
        std::vector<float> range(px), normal(px * 3);
        std::vector<uint8_t> flags(px);
        DsrtGBuffer g;
        std::memset(&g, 0, sizeof g);
        g.range = range.data(); g.normal = normal.data(); g.flags = flags.data();
        if (dsrt_render_gbuffer_to_host(ctx, &d, &g, nullptr) != DSRT_OK) return fail("rendering the G-buffer");
        if (dsrt_write_pfm((base + "_range.pfm").c_str(), range.data(), width, height, 1) != DSRT_OK ||
            dsrt_write_pfm((base + "_normal.pfm").c_str(), normal.data(), width, height, 3) != DSRT_OK) return fail("writing the G-buffer");
        if (!write_mask_pgm(base + "_mask.pgm", flags, width, height, DSRT_GB_HIT) || !write_mask_pgm(base + "_sunlit.pgm", flags, width, height, DSRT_GB_SUN_VISIBLE)) {
            std::fprintf(stderr, "dsrt_render: cannot write the masks of %s\n", base.c_str());
            return 1;
        }
        std::printf("Saved %s_{range,normal}.pfm, %s_{mask,sunlit}.pgm\n", base.c_str(), base.c_str());
        return 0;
    };

    // --coverage: the sub-pixel coverage of the frame the context's camera, sun and body poses are set to; with --body one class per body
    auto write_coverage = [&](const std::string& base) -> int {
        const int nb = bodies.empty() ? 0 : (int)bodies.size() + 1;
        std::vector<float> a(px), sa(px), planes((size_t)nb * px);
        std::vector<uint8_t> ch((size_t)nb * px);
        DsrtCoverageClasses cl;
        std::memset(&cl, 0, sizeof cl);
        cl.count = nb;
        for (int b = 0; b < nb; ++b) if (dsrt_host_scene_body_range(hs, b, &cl.first[b], &cl.num[b]) != DSRT_OK) return fail("asking for a body's triangles");
        DsrtCoverage cv;
        std::memset(&cv, 0, sizeof cv);
        cv.alpha = a.data(); cv.sun_alpha = sa.data();
        if (nb) cv.class_hits = ch.data();
        if (dsrt_render_coverage_to_host(ctx, &d, &cov_desc, nb ? &cl : nullptr, &cv, nullptr) != DSRT_OK) return fail("rendering the coverage");
        if (dsrt_write_pfm((base + "_alpha.pfm").c_str(), a.data(), width, height, 1) != DSRT_OK ||
            dsrt_write_pfm((base + "_sun_alpha.pfm").c_str(), sa.data(), width, height, 1) != DSRT_OK) return fail("writing the coverage");
        if (nb) {
            const float fn = (float)(cov_desc.pattern == DSRT_COVERAGE_GRID ? cov_desc.samples * cov_desc.samples : cov_desc.samples);
            for (int b = 0; b < nb; ++b)
                for (size_t i = 0; i < px; ++i) planes[(size_t)b * px + i] = (float)ch[i * (size_t)nb + (size_t)b] / fn;
            if (dsrt_write_pfm((base + "_body_alpha.pfm").c_str(), planes.data(), width, height * nb, 1) != DSRT_OK) return fail("writing the bodies' coverage");
        }
        std::printf("Saved %s_{alpha,sun_alpha%s}.pfm\n", base.c_str(), nb ? ",body_alpha" : "");
        return 0;
    };

    // --sensor, --stars or --lens without --denoise or --upscale: the plain mean of the frame's samples as its linear image (the denoiser with 0 iterations); with --variance its variance.
    DsrtDenoise dn_mean = dn;
    dn_mean.iterations = 0;
    if (wants_linear && !frame_step) frame_step = [&](size_t, const std::string& base) -> int {
        DsrtStats st;
        if (dsrt_render_denoised_to_host(ctx, &d, &dn_mean, img.data(), nullptr, lin, variance ? var.data() : nullptr, &st) != DSRT_OK) return fail("rendering the linear frame");
        const std::string path = base + ext;
        if (!write_image(path, img.data())) return fail("writing the frame");
        if (!write_var(base)) return fail("writing the variance");
        std::printf("kernel %.3f ms\nSaved %s%s\n", st.kernel_ms, path.c_str(), variance ? " and _var.pfm" : "");
        return 0;
    };
    // --stars: the star field added to the linear image the frame's step left (include/dsrt.h, POINT SOURCES), the catalogue through the frame's pose
    const size_t n_stars = stars_spec.flux.size() / 3;
    std::vector<float> star_dirs(stars ? n_stars * 3 : 0), star_xy(stars ? n_stars * 2 : 0), star_layer(stars ? sensor_linear.size() : 0), star_sum(star_layer.size());
    std::vector<uint8_t> star_status(stars ? n_stars : 0);
    auto write_stars = [&](size_t id, const std::string& base) -> int {
        DsrtRenderDesc sd = d;
        sd.width = sensor_w; sd.height = sensor_h;
        if (n_stars && dsrt_pose_dirs_to_model(&poses[id], (int)n_stars, stars_spec.world_dirs.data(), star_dirs.data()) != DSRT_OK) return fail("bringing the stars into the model frame");
        DsrtStars in;
        std::memset(&in, 0, sizeof in);
        in.count = (int)n_stars; in.occlusion = stars_spec.occlusion; in.dir = star_dirs.data(); in.flux = stars_spec.flux.data(); in.linear_in = lin;
        const DsrtStarsOut out{star_layer.data(), star_sum.data(), n_stars ? star_xy.data() : nullptr, n_stars ? star_status.data() : nullptr};
        if (dsrt_render_stars_to_host(ctx, &sd, &in, &out, nullptr) != DSRT_OK) return fail("rendering the star field");
        sensor_linear = star_sum;                                   // what --sensor sees
        if (dsrt_write_pfm((base + "_stars.pfm").c_str(), star_layer.data(), sensor_w, sensor_h, 3) != DSRT_OK) return fail("writing the star layer");
        FILE* f = std::fopen((base + "_stars.txt").c_str(), "w");
        if (!f) { std::fprintf(stderr, "dsrt_render: cannot write %s_stars.txt\n", base.c_str()); return 1; }
        size_t visible = 0;
        for (size_t i = 0; i < n_stars; ++i) {
            std::fprintf(f, "%zu %.9g %.9g %u\n", i, (double)star_xy[2 * i], (double)star_xy[2 * i + 1], (unsigned)star_status[i]);
            visible += (star_status[i] >> 1) & 1u;
        }
        if (std::fclose(f) != 0) { std::fprintf(stderr, "dsrt_render: short write to %s_stars.txt\n", base.c_str()); return 1; }
        std::printf("stars: %zu of %zu visible at %d x %d%s\nSaved %s_stars.pfm, %s_stars.txt\n", visible, n_stars, sensor_w, sensor_h, stars_spec.occlusion ? "" : ", occlusion off",
                    base.c_str(), base.c_str());
        return 0;
    };
    // --lens: the linear image the frame's step (and --stars) left, through the lens (include/dsrt.h, LENS MODEL); `q` indexes the frame's camera
    const size_t lens_px = lens ? (size_t)sensor_w * sensor_h : 0;
    std::vector<float> lens_image(lens_px * 3), lens_xy(lens_px * 2), lens_map(lens_px * 3), star_lens_xy(lens && stars ? star_xy.size() : 0);
    std::vector<uint8_t> lens_status(lens_px), star_lens_ok(lens && stars ? n_stars : 0);
    auto write_lens = [&](size_t q, const std::string& base) -> int {
        DsrtRenderDesc sd = d;
        sd.width = sensor_w; sd.height = sensor_h;
        float k[4];
        if (dsrt_lens_intrinsics_from_camera(&cams[q], sensor_w, sensor_h, k) != DSRT_OK) return fail("taking the camera's intrinsics");
        DsrtLens& p = lens_spec.p;
        p.src_width = sensor_w; p.src_height = sensor_h; p.channels = 3;
        p.src_fx = k[0]; p.src_fy = k[1]; p.src_cx = k[2]; p.src_cy = k[3];
        p.fx = (float)(k[0] * lens_spec.zoom); p.fy = (float)(k[1] * lens_spec.zoom); p.cx = k[2]; p.cy = k[3];
        const DsrtLensOut out{lens_image.data(), lens_xy.data(), lens_status.data()};
        if (dsrt_lens_apply_to_host(ctx, &sd, lin, &p, &out) != DSRT_OK) return fail("applying the lens model");
        size_t inverted = 0;
        for (size_t i = 0; i < lens_px; ++i) {
            lens_map[3 * i] = lens_xy[2 * i]; lens_map[3 * i + 1] = lens_xy[2 * i + 1]; lens_map[3 * i + 2] = (float)lens_status[i];
            inverted += lens_status[i] & DSRT_LENS_INVERTED;
        }
        if (dsrt_write_pfm((base + "_lens.pfm").c_str(), lens_image.data(), sensor_w, sensor_h, 3) != DSRT_OK ||
            dsrt_write_pfm((base + "_lens_map.pfm").c_str(), lens_map.data(), sensor_w, sensor_h, 3) != DSRT_OK) return fail("writing the warped frame");
        sensor_linear = lens_image;                                 // what --sensor sees
        std::printf("lens: %d x %d, filter %d, %zu of %zu pixels have a source\nSaved %s_lens.pfm, %s_lens_map.pfm\n", sensor_w, sensor_h, p.filter, inverted, lens_px,
                    base.c_str(), base.c_str());
        if (!stars) return 0;
        if (dsrt_lens_distort_points(&p, (int)n_stars, star_xy.data(), star_lens_xy.data(), star_lens_ok.data()) != DSRT_OK) return fail("distorting the star centroids");
        FILE* f = std::fopen((base + "_stars_lens.txt").c_str(), "w");
        if (!f) { std::fprintf(stderr, "dsrt_render: cannot write %s_stars_lens.txt\n", base.c_str()); return 1; }
        for (size_t i = 0; i < n_stars; ++i) {
            const bool has = (star_status[i] & 1u) && star_lens_ok[i];           // projected by the pinhole, and finite through the lens
            std::fprintf(f, "%zu %.9g %.9g %u\n", i, has ? (double)star_lens_xy[2 * i] : 0.0, has ? (double)star_lens_xy[2 * i + 1] : 0.0, (unsigned)star_status[i]);
        }
        if (std::fclose(f) != 0) { std::fprintf(stderr, "dsrt_render: short write to %s_stars_lens.txt\n", base.c_str()); return 1; }
        std::printf("Saved %s_stars_lens.txt\n", base.c_str());
        return 0;
    };
    // --sensor: the detector over the linear image the frame's step left (include/dsrt.h, SENSOR MODEL); `frame` is the frame's index in the pose file
    sensor_spec.p.psf = sensor_spec.taps.empty() ? nullptr : sensor_spec.taps.data();
    const size_t sensor_px = (size_t)sensor_w * sensor_h, sensor_planes = sensor_spec.p.mono ? 1 : 3;
    std::vector<uint16_t> sensor_dn(sensor ? sensor_px * sensor_planes : 0);
    std::vector<uint8_t> sensor_rgb(sensor ? sensor_px * 3 : 0);
    auto write_sensor = [&](size_t id, const std::string& base) -> int {
        DsrtRenderDesc sd = d;
        sd.width = sensor_w; sd.height = sensor_h;
        sensor_spec.p.frame = (uint32_t)id;
        if (dsrt_sensor_apply_to_host(ctx, &sd, lin, &sensor_spec.p, sensor_dn.data(), nullptr, sensor_rgb.data()) != DSRT_OK) return fail("applying the sensor model");
        const std::string raw_path = base + (sensor_spec.p.mono ? "_raw.pgm" : "_raw.ppm");
        if (dsrt_write_pnm16(raw_path.c_str(), sensor_dn.data(), sensor_w, sensor_h, (int)sensor_planes, (1 << sensor_spec.p.bits) - 1) != DSRT_OK ||
            dsrt_write_png((base + "_sensor.png").c_str(), sensor_rgb.data(), sensor_w, sensor_h) != DSRT_OK) return fail("writing the raw frame");
        std::printf("sensor: %d x %d, %d bits, %s, frame %u\nSaved %s, %s_sensor.png\n", sensor_w, sensor_h, sensor_spec.p.bits, sensor_spec.p.mono ? "mono" : "colour",
                    sensor_spec.p.frame, raw_path.c_str(), base.c_str());
        return 0;
    };

    // --body: a batch launch has one scene and therefore one set of poses (include/dsrt.h), so a run with bodies renders one launch per frame
    if (!bodies.empty() && !frame_step) frame_step = [&](size_t, const std::string& base) -> int {
        DsrtStats st;
        if (dsrt_render_to_host(ctx, &d, img.data(), nullptr, &st) != DSRT_OK) return fail("rendering");
        const std::string path = base + ext;
        if (!write_image(path, img.data())) return fail("writing the frame");
        std::printf("kernel %.3f ms\nSaved %s\n", st.kernel_ms, path.c_str());
        return gbuffer ? write_gbuffer(base) : 0;
    };

    for (size_t q = 0; frame_step && q < ids.size(); ++q) {
        if (q < body_poses.size()) {
            float ms = 0.0f;
            if (dsrt_scene_set_body_poses(ctx, 1, (int)bodies.size(), body_poses[q].data(), nullptr, &ms) != DSRT_OK) return fail("posing the bodies");
            std::printf("bodies posed on the device in %.3f ms\n", ms);
        }
        if (dsrt_scene_set_camera_sun(ctx, &cams[q], suns.data() + 3 * q) != DSRT_OK) return fail("setting the camera");
        if (const int rc = frame_step(q, frame_base(ids[q]))) return rc;
        if (stars) if (const int rc = write_stars(ids[q], frame_base(ids[q]))) return rc;
        if (lens) if (const int rc = write_lens(q, frame_base(ids[q]))) return rc;
        if (sensor) if (const int rc = write_sensor(ids[q], frame_base(ids[q]))) return rc;
        if (coverage) if (const int rc = write_coverage(frame_base(ids[q]))) return rc;
    }
    size_t per_launch = 32;
    while (per_launch > 1 && (unsigned long long)per_launch * width * height * (rng_mode == 1 ? 16ull : 1ull) >= (1ull << 32)) per_launch /= 2;
    std::vector<uint8_t> fb(frame_step ? 0 : image_bytes * std::min(per_launch, std::max<size_t>(ids.size(), 1)));
    for (size_t k = 0; !frame_step && k < ids.size(); k += per_launch) {
        const size_t n = std::min(per_launch, ids.size() - k);
        DsrtStats st;
        if (dsrt_render_batch_to_host(ctx, &d, (int)n, cams.data() + k, suns.data() + 3 * k, fb.data(), &st) != DSRT_OK) return fail("rendering");
        std::printf("\nframes %zu..%zu: kernel %.3f ms (%.1f Msamples/s)\n", ids[k], ids[k + n - 1], st.kernel_ms, (double)n * width * height * spp / (st.kernel_ms * 1e3));
        for (size_t q = 0; q < n; ++q) {
            const std::string base = frame_base(ids[k + q]), path = base + ext;
            if (!write_image(path, fb.data() + q * image_bytes)) return fail("writing the frame");
            std::printf("Saved %s\n", path.c_str());
            if (gbuffer || coverage) {
                // (the batch launch above took camera and sun as arguments: the context's are set to this frame's)
                if (dsrt_scene_set_camera_sun(ctx, &cams[k + q], suns.data() + 3 * (k + q)) != DSRT_OK) return fail("setting the camera");
                if (gbuffer) if (const int rc = write_gbuffer(base)) return rc;
                if (coverage) if (const int rc = write_coverage(base)) return rc;
            }
        }
    }
    dsrt_ctx_destroy(ctx);
    dsrt_host_scene_destroy(hs);
    std::printf("Done.\n");
    return 0;
}
