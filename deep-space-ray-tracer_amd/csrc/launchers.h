// launchers.h -- the one declaration of every host-side launcher that crosses a translation unit.  device_api.hip calls them; every .hip file that defines
// one includes this header too, so a definition is checked against its declaration where it is compiled.
#pragma once

#include "device_layout.h"
#include "lens_math.h"

namespace dsrt {

// Which instantiation of dsrt_render_kernel a launch wants (render_kernel.hip: launch_render picks it and refuses what is not built).
//   count, checked: the counting / checked builds (never LEAN)      anyhit: shadow rays stop at the first accepted triangle
//   lean: a scene of Lambertian triangles only (path_machine.h)     sets, moments: the rng_mode 1 launches of dsrt_render_accumulate
//   listed: dsrt_render_listed_kernel -- a sets launch over the lists of active pixels (dsrt_render_accumulate_masked); never count
struct RenderVariant { int rng_mode; bool count, checked, anyhit, lean, sets, moments, listed; };

// The launchers of render_kernel.hip.  That file is compiled twice -- with the deterministic sin / cos / pow shared with the CPU oracle, and against the device
// math library's (DsrtRenderDesc.math_mode 1, namespace devlibm) -- and each compilation exports its launchers as one table.
struct RenderLaunchers {
    hipError_t (*launch_render)(const RenderArgs& a, const RenderVariant& v, int blocks, hipStream_t stream);
    hipError_t (*launch_render_batch)(const RenderArgs& a, int rng_mode, int blocks, bool lean, hipStream_t stream);
    hipError_t (*launch_probe)(const RenderArgs& a, int blocks, bool lean, hipStream_t stream);
};
const RenderLaunchers& compiled_render_launchers();
namespace devlibm { const RenderLaunchers& compiled_render_launchers(); }
const RenderLaunchers& render_launchers(bool device_libm);          // api_render.hip: the table of one of the two

// schedule_kernel.hip: the scheduling pre-pass
hipError_t launch_tile_order(const DeviceScene& S, const FrameParams& P, uint32_t* cost, uint32_t* order, uint32_t* sched, uint32_t items_per_pixel,
                             uint32_t resident_lanes, bool cull, hipStream_t stream, const BatchFrame* batch = nullptr, uint32_t frames = 1, uint32_t stride = 0);
// (dsrt_selftest_tile_order: the order kernel alone, one frame, on cost words the caller supplies -- no cost kernel in front)
hipError_t launch_tile_order_arrays(const uint32_t* cost, uint32_t* order, int n, int tile, uint32_t* sched, uint32_t items_per_pixel, uint32_t resident_lanes, int spp,
                                    hipStream_t stream);
hipError_t launch_tile_reorder(const uint32_t* work, uint32_t* order, uint32_t* tmp, const uint32_t* sched, hipStream_t stream);
hipError_t launch_batch_table(BatchFrame* table, const uint32_t* sched, uint32_t sched_stride, uint32_t frames, uint32_t tt, int rng_mode, int spp, int light_chunk_len,
                              uint32_t* total_items, hipStream_t stream);

// sample_set_kernel.hip: the lists of a masked accumulate launch (with its update of the sample counts), the counts of an unmasked pass, the convergence test ...
hipError_t launch_pixel_list(const FrameParams& P, const uint32_t* order, const uint32_t* sched, const uint8_t* mask, uint32_t* list, uint32_t* list_len,
                             uint32_t* n, uint32_t count, hipStream_t stream);
hipError_t launch_add_count(uint32_t* n, uint32_t count, size_t n_pixels, hipStream_t stream);
hipError_t launch_select_unconverged(const unsigned long long* sums, const unsigned long long* sums_sq, const uint32_t* counts, size_t n_pixels, float rel_tol, float floor_,
                                     uint32_t n_min, uint32_t n_max, uint8_t* mask, uint32_t* n_active, hipStream_t stream);
// ... and the resolve of the sums to an image, with n = samples_done for every pixel or each pixel's own counts[i]; the outputs that are not null are written
hipError_t launch_resolve(const unsigned long long* sums, int samples_done, float inv_gamma, bool device_libm, size_t n_pixels, uint8_t* out_rgb8, float* out_f32,
                          const unsigned long long* sums_sq, float* out_var, hipStream_t stream);
hipError_t launch_resolve_counts(const unsigned long long* sums, const uint32_t* counts, float inv_gamma, bool device_libm, size_t n_pixels, uint8_t* out_rgb8,
                                 float* out_f32, const unsigned long long* sums_sq, float* out_var, hipStream_t stream);

// selftest_kernel.hip: tile de-interleave, the drop-in layer's content hash and the self-test hooks
hipError_t launch_deinterleave(const uint8_t* gathered, uint8_t* image, int W, int H, int tile, int tiles_x, int shard_count,
                               size_t shard_stride_bytes, hipStream_t stream);
hipError_t launch_content_hash(const uint32_t* words, size_t n_words, uint64_t salt, uint64_t* d_hash2, hipStream_t stream);
hipError_t launch_math(int fn, const float* x, float y, float* out, int n, hipStream_t stream);
hipError_t launch_devkat(int fn, const float* in, float* out, int n, hipStream_t stream);
hipError_t launch_philox(unsigned long long seed, unsigned long long sub, int n, uint32_t* ours, uint32_t* theirs, hipStream_t stream);

hipError_t launch_gbuffer(const GBufferArgs& a, int tiles, hipStream_t stream);                                  // gbuffer_kernel.hip
hipError_t launch_raycast(const RaycastArgs& a, bool any_hit, int blocks, hipStream_t stream);                   // raycast_kernel.hip
hipError_t launch_coverage(const CoverageArgs& a, int blocks, hipStream_t stream);                               // coverage_kernel.hip: one wave per 64 / a.n pixels

// denoise_kernel.hip (include/dsrt.h, DENOISER).  The filter's working memory, one 16-byte record per pixel each: {c.rgb, L(c)} and {v.rgb, L(v)} twice (the
// iterations ping-pong between [0] and [1]), and the guides {N, range}, {X, filterable}, {A, 0}.  prepare fills cl[0], vl[0] and the guides; an a-trous launch
// reads cl / vl[src] and writes [src ^ 1]; output reads [src].
struct DenoiseBuffers { float4* cl[2]; float4* vl[2]; float4* nr; float4* xf; float4* al; };
hipError_t launch_denoise_prepare(const unsigned long long* sums, const unsigned long long* sums_sq, int samples_done, const uint32_t* counts, const float* normal,
                                  const float* position, const float* albedo, const float* range, size_t n_pixels, const DenoiseBuffers& b, hipStream_t stream);
hipError_t launch_denoise_atrous(const DenoiseBuffers& b, int src, int W, int H, int step, int normal_power_log2, float sigma_l, float sigma_z, float sigma_a,
                                 hipStream_t stream);
hipError_t launch_denoise_output(const DenoiseBuffers& b, int src, size_t n_pixels, float inv_gamma, bool device_libm, uint8_t* out_rgb8, float* out_f32, float* out_linear,
                                 float* out_var, hipStream_t stream);
// ... with COVERAGE DEMODULATION (include/dsrt.h): `alpha` one float per pixel, never null here (a call without one uses the two above: their kernels are the
// HAS_ALPHA = false instantiations of the same templates).  prepare divides the filterable pixels' c and v by a and a*a, output multiplies them back.
hipError_t launch_denoise_prepare_coverage(const unsigned long long* sums, const unsigned long long* sums_sq, int samples_done, const uint32_t* counts, const float* normal,
                                           const float* position, const float* albedo, const float* range, const float* alpha, float alpha_min, size_t n_pixels,
                                           const DenoiseBuffers& b, hipStream_t stream);
hipError_t launch_denoise_output_coverage(const DenoiseBuffers& b, int src, const float* alpha, size_t n_pixels, float inv_gamma, bool device_libm, uint8_t* out_rgb8,
                                          float* out_f32, float* out_linear, float* out_var, hipStream_t stream);

// temporal_kernel.hip (include/dsrt.h, TEMPORAL ACCUMULATION): between prepare and the first a-trous launch.  cl / vl are DenoiseBuffers' [0], blended in place;
// prev (null = no previous frame) and next are the caller's histories, four float4 per pixel; cam = the previous GPUCamera's origin, lower_left_corner,
// horizontal, vertical, u, v, w; counts / samples_done as prepare's.
struct TemporalArgs {
    float4* cl; float4* vl; const float4* nr; const float4* xf;
    const float4* prev; float4* next; float* prev_xy; float* weight;
    const uint32_t* counts; int samples_done, width, height;
    float cam[21];
    float alpha_min, normal_cos_min, plane_tol, min_support;
};
// The same with the motion stage (include/dsrt.h, TEMPORAL ACCUMULATION WITH BODIES), a second kernel argument beside TemporalArgs, which stays as it is: the
// G-buffer's prim_id, the optional X' output, per body >= 1 its triangle range [first, first + count) (zero for a body not given: an empty range), bit b of `moved`
// set where body b's poses differ, and per body six float4 -- the cur pose's three rows {r0 r1 r2 t}, then the prev pose's (host/body_motion.cpp, BodyMotionTable).
constexpr int kMaxBodies = 16;             // DSRT_MAX_BODIES
struct BodyMotionArgs {
    const int* prim_id; float* prev_position;
    int first[kMaxBodies], count[kMaxBodies];
    uint32_t moved;
    float4 poses[kMaxBodies * 6];
};
// ... and with the sun state (include/dsrt.h, TEMPORAL ACCUMULATION THAT FOLLOWS SHADING), a third kernel argument; the other two stay as they are.  flags: the
// current G-buffer's u8 channel; status: the optional byte per pixel; edge_guard 0 or 1.  mo.prim_id null: a static scene (every pixel body 0; moved = 0, and
// prev_position null).
struct ShadingArgs { const uint8_t* flags; uint8_t* status; int edge_guard; };
// One launcher picks the kernel: null mo and null sh the static one (dsrt_temporal_kernel), mo alone the one with the motion stage, sh the one with the sun state
// as well (mo is required then: all zero for a static scene).
hipError_t launch_temporal(const TemporalArgs& a, const BodyMotionArgs* mo, const ShadingArgs* sh, hipStream_t stream);

// upscale_kernel.hip (include/dsrt.h, UPSCALER).  The LOW-resolution frame packed for the taps, one 16-byte record per low-resolution pixel each: {c.rgb, range},
// {v.rgb, flags as a bit pattern}, {N, 0}, {X, 0}, {A, 0}.  pack fills them (var and flags may be null: zeros); the upscale launch reads them and the OUTPUT
// resolution's guides as the caller has them, and writes the outputs that are not null.
struct UpscaleRecords { float4* cr; float4* vf; float4* nn; float4* xx; float4* aa; };
struct UpscaleArgs {
    const float4* cr; const float4* vf; const float4* nn; const float4* xx; const float4* aa;
    const float* hi_normal; const float* hi_position; const float* hi_albedo; const float* hi_range; const uint8_t* hi_flags;
    uint8_t* out_rgb8; float* out_f32; float* out_linear; float* out_var; float* out_support;
    int w, h, W, H;                      // low resolution, output resolution
    int normal_power_log2, use_sun, lo_has_flags;
    float sigma_z, sigma_a, inv_gamma;
};
hipError_t launch_upscale_pack(const float* linear, const float* var, const float* normal, const float* position, const float* albedo, const float* range,
                               const uint8_t* flags, size_t n_pixels, const UpscaleRecords& r, hipStream_t stream);
hipError_t launch_upscale(const UpscaleArgs& a, bool device_libm, hipStream_t stream);
// ... with coverage (include/dsrt.h, COVERAGE-AWARE UPSCALER): `alpha` / hi_alpha one float per low-resolution / output pixel, never null here (a call without them
// uses the two above: their kernels are the HAS_ALPHA = false instantiations of the same bodies).  pack keeps the low-resolution alpha in the normal record's spare
// word, {N, alpha}: working memory stays five records.  out_level (optional): one byte per output pixel, the level that produced it.
struct UpscaleCoverageArgs { UpscaleArgs up; const float* hi_alpha; uint8_t* out_level; float alpha_min; };
hipError_t launch_upscale_pack_coverage(const float* linear, const float* var, const float* normal, const float* position, const float* albedo, const float* range,
                                        const uint8_t* flags, const float* alpha, size_t n_pixels, const UpscaleRecords& r, hipStream_t stream);
hipError_t launch_upscale_coverage(const UpscaleCoverageArgs& a, bool device_libm, hipStream_t stream);

// sensor_kernel.hip (include/dsrt.h, SENSOR MODEL).  in: the linear frame, W*H*3 floats; psf: psf_size x psf_size taps on the DEVICE (null = no blur, psf_size then
// unused); the outputs that are not null are written (at least one is), C = 1 (`mono`) or 3 planes per pixel in out_dn and out_signal, always 3 bytes in out_rgb8.
// The rest is DsrtSensor's, the seed as its two Philox key words.
struct SensorArgs {
    const float* in; const float* psf;
    uint16_t* out_dn; float* out_signal; uint8_t* out_rgb8;
    int W, H, psf_size;
    float gain_e, prnu, dark_e, dsnu_e, read_e, full_well_e, e_per_dn, offset_dn;
    int bits, noise;
    uint32_t seed_lo, seed_hi, frame;
};
hipError_t launch_sensor(const SensorArgs& a, bool mono, hipStream_t stream);

// stars_kernel.hip (include/dsrt.h, POINT SOURCES).  dir / flux: count x 3 floats; cam: the context's GPUCamera's origin, lower_left_corner, horizontal, vertical,
// u, v, w; list (count words) and list_len (one word, zero at launch): the projected stars' indices; acc: W*H*3 sums, zero at launch and zero again after it, null when neither layer nor
// linear_out is asked for (nothing is deposited or resolved then); the outputs that are not null are written; status: the walk's kFlag* bits.
struct StarsArgs {
    DeviceScene scene;
    const float* dir; const float* flux; const float* linear_in;
    int count, width, height, occlusion;
    int stack_entries;         // LDS stack entries per lane the launch provides (>= the tree's stack_need)
    float cam[21];
    uint32_t* list; uint32_t* list_len;
    unsigned long long* acc;
    float* layer; float* linear_out; float* xy; uint8_t* star_status;
    uint32_t* status;
};
hipError_t launch_stars(const StarsArgs& a, hipStream_t stream);             // project, deposit, resolve: three launches in stream order

// lens_kernel.hip (include/dsrt.h, LENS MODEL).  src: the pinhole frame, src_w*src_h*channels 32-bit words (floats for filters 1 and 2); the outputs that are not
// null are written (at least one is): out_image W*H*channels words, out_src_xy W*H*2 floats, out_status W*H bytes.  The rest is DsrtLens's.
struct LensArgs {
    const uint32_t* src;
    uint32_t* out_image; float* out_src_xy; uint8_t* out_status;
    int W, H, src_w, src_h;
    float fx, fy, cx, cy, src_fx, src_fy, src_cx, src_cy;
    LensCoeffs c;
    float v1, v2, v3;
    int cos4, clamp_zero;
    uint32_t fill_bits;
};
hipError_t launch_lens(const LensArgs& a, int channels, int filter, hipStream_t stream);      // dsrt_lens_kernel<channels, filter>

// bodies_kernel.hip (include/dsrt.h, MOVABLE RIGID BODIES). What a pose update reads and writes: the three arrays of the resident scene it rewrites in place, and what
// dsrt_scene_upload_bodies made resident beside them.  A movable ENTRY is a pair record of tri_pairs that holds triangles of a body >= 1; entries are sorted by body.
struct BodiesView {
    float4* pairs; float4* tri_pairs; float4* tri_shade;     // the resident scene's (device_layout.h)
    const int2* big_leaves;
    const float4* rest_v;      // per entry, 5 x float4: A's v0 v1 v2 (9 floats), B's (9 floats), the pair record's index, body | (has a B triangle) << 8 -- as int bits
    const float4* rest_n;      // per entry, 5 x float4: A's n0 n1 n2, B's, two unused
    float4* pair_box;          // per pair record of the WHOLE scene, 2 x float4: (lo.xyz, -) (hi.xyz, -) of its one or two triangles, unpadded; the static ones are filled at upload
    const float* poses;        // kMaxBodies x 12
    const float* pads;         // kMaxBodies
    const int2* refit;         // {node record, body} of every internal node of a movable subtree, deepest depth first
    const int4* chain;         // {node record, body of the left child, body of the right child or 0 where that is the next top node, -}, T0 first
    float* root_box;           // 6 floats: lo, hi of the scene
    int n_chain, root_ref, root_body;
    int num_pairs, num_tri_pairs, num_big_leaves;
};
hipError_t launch_bodies_transform(const BodiesView& b, int first_entry, int entries, hipStream_t stream);
hipError_t launch_bodies_refit(const BodiesView& b, int first, int count, hipStream_t stream);       // a range of BodiesView::refit: one depth
hipError_t launch_bodies_chain(const BodiesView& b, hipStream_t stream);

}  // namespace dsrt
