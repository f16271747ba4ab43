/*
 * dsrt.h -- C ABI of libdsrt_hip.so, the MI355X-native renderer behind the Deep-Space-Ray-Tracer
 * host API.  Plain C types only: pointers, sizes, PODs from dsrt_scene_abi.h.  No torch types, no
 * C++ classes.  Every entry point names the reference interface it stands in for
 * (file:line relative to the reference repository).
 *
 * Error model: every int-returning function returns DSRT_OK (0) or a negative DSRT_ERR_*; the text
 * of the last failure on the calling thread is available from dsrt_last_error().  The reference
 * prints to stderr and returns void (src/gpu_render.cu:1053-1094, src/gpu_scene_builder.cpp:27-34);
 * the drop-in wrappers at the bottom keep that behaviour on top of these functions.
 *
 * Threading: a DsrtHostScene or DsrtContext may be used by one thread at a time.
 */
#ifndef DSRT_H
#define DSRT_H

#include "dsrt_scene_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DSRT_OK               0
#define DSRT_ERR_INVALID     -1   /* bad argument                                              */
#define DSRT_ERR_IO          -2   /* file could not be read / written                          */
#define DSRT_ERR_HIP         -3   /* a HIP runtime call failed                                 */
#define DSRT_ERR_NO_DEVICE   -4   /* no usable gfx950 device                                   */
#define DSRT_ERR_BVH_DEPTH   -5   /* BVH deeper than the 64-entry stack of src/gpu_render.cu:399 */
#define DSRT_ERR_NO_SCENE    -6   /* render before upload                                      */
#define DSRT_ERR_DEVICE_FLAG -7   /* the kernel raised its checked-mode status word            */
#define DSRT_ERR_NOMEM       -8   /* host allocation failed (no C++ exception crosses this ABI) */
#define DSRT_ERR_COMM        -9   /* an RCCL call failed                                         */

const char* dsrt_last_error(void);
/* ABI version: THE one place it is written.  Bumped on any signature, struct or flag change (3 = round 2: DsrtStats grew,
 * dsrt_render_batch, dsrt_multi_*; 4 = round 3: DsrtRenderDesc.tune[3] pruned to the switches a host may need, reserved bits
 * refused; dsrt_selftest_devkat, dsrt_microbench_valu; 5 = DsrtRenderDesc.math_mode appended;
 * 6 = dsrt_host_scene_add_texture_file; 7 = round 4: dsrt_microbench_copy, dsrt_sizeof, dsrt_dev_set_experiment, dsrt_selftest_poke_node_word, dsrt_ctx_set_certified_tree, DsrtStats grew; 8 = DsrtGBuffer, dsrt_render_gbuffer, dsrt_render_gbuffer_to_host, dsrt_write_pfm; purely additive since, version kept: DsrtRays, DsrtRayHits, dsrt_trace_rays, dsrt_trace_rays_to_host, dsrt_pose_points_to_model, dsrt_pose_dirs_to_model, DsrtAccum, dsrt_render_accumulate, dsrt_render_accumulate_to_host, dsrt_resolve_accumulated, dsrt_resolve_accumulated_to_host, DSRT_SIZEOF_ACCUM, DsrtAdaptive, DsrtAdaptiveStats, dsrt_render_accumulate_masked, dsrt_render_accumulate_masked_to_host, dsrt_select_unconverged, dsrt_resolve_accumulated_counts, dsrt_render_adaptive, dsrt_render_adaptive_to_host, DSRT_SIZEOF_ADAPTIVE, DSRT_SIZEOF_ADAPTIVE_STATS, DsrtDenoiseGuides, DsrtDenoise, dsrt_denoise_defaults, dsrt_denoise_accumulated, dsrt_denoise_accumulated_to_host, dsrt_render_denoised_to_host, DSRT_SIZEOF_DENOISE_GUIDES, DSRT_SIZEOF_DENOISE, DsrtTemporal, dsrt_temporal_defaults, dsrt_denoise_temporal, dsrt_denoise_temporal_to_host, dsrt_render_denoised_temporal_to_host, DSRT_SIZEOF_TEMPORAL, DsrtUpscaleGuides, DsrtUpscale, dsrt_upscale_defaults, dsrt_upscale_guided, dsrt_upscale_guided_to_host, dsrt_render_upscaled_to_host, DSRT_SIZEOF_UPSCALE_GUIDES, DSRT_SIZEOF_UPSCALE, DSRT_MAX_BODIES, dsrt_host_scene_begin_body, dsrt_host_scene_body_count, dsrt_host_scene_body_range, dsrt_host_scene_build_bvh_bodies, dsrt_host_scene_set_body_poses, dsrt_scene_upload_bodies, dsrt_scene_set_body_poses, dsrt_ctx_body_count, dsrt_ctx_body_update_ms, dsrt_selftest_read_scene_words, DsrtBodyMotion, dsrt_body_motion_host, dsrt_denoise_temporal_bodies, dsrt_denoise_temporal_bodies_to_host, dsrt_ctx_set_temporal_bodies, dsrt_ctx_temporal_bodies, DSRT_SIZEOF_BODY_MOTION, DsrtCoverageDesc, DsrtCoverageClasses, DsrtCoverage, dsrt_coverage_defaults, dsrt_render_coverage, dsrt_render_coverage_to_host, dsrt_denoise_coverage_alpha_min, dsrt_denoise_accumulated_coverage, dsrt_denoise_accumulated_coverage_to_host, dsrt_render_denoised_coverage_to_host, DSRT_SIZEOF_COVERAGE_DESC, DSRT_SIZEOF_COVERAGE, DSRT_SIZEOF_COVERAGE_CLASSES, dsrt_selftest_read_schedule, dsrt_selftest_tile_order, dsrt_selftest_tile_reorder, dsrt_selftest_batch_table, dsrt_upscale_coverage_alpha_min, dsrt_upscale_guided_coverage, dsrt_upscale_guided_coverage_to_host, dsrt_render_upscaled_coverage_to_host, DsrtSensor, dsrt_sensor_defaults, dsrt_sensor_psf_gaussian, dsrt_sensor_apply, dsrt_sensor_apply_to_host, dsrt_write_pnm16, DSRT_SIZEOF_SENSOR, DsrtStars, DsrtStarsOut, dsrt_render_stars, dsrt_render_stars_to_host, dsrt_stars_from_catalog, dsrt_stars_synthetic_catalog, DSRT_SIZEOF_STARS, DSRT_SIZEOF_STARS_OUT, DsrtLens, DsrtLensOut, dsrt_lens_defaults, dsrt_lens_apply, dsrt_lens_apply_to_host, dsrt_lens_distort_points, dsrt_lens_intrinsics_from_camera, DSRT_SIZEOF_LENS, DSRT_SIZEOF_LENS_OUT).  dsrt_abi_version() returns the value the library was compiled with;
 * bindings parse this line (capi.header_abi_version) and compare. */
#define DSRT_ABI_VERSION 8
int dsrt_abi_version(void);
/* sizeof of the structs that cross this ABI, as the LIBRARY was compiled: a binding that mirrors them by hand (ctypes, cgo, JNA ...) compares its own sizes with
 * these at load time, so that a struct that grew in the header and the library but not in the binding is refused instead of silently mis-laid.  0 = unknown. */
#define DSRT_SIZEOF_RENDER_DESC 0
#define DSRT_SIZEOF_STATS       1
#define DSRT_SIZEOF_GPU_SCENE   2
#define DSRT_SIZEOF_GPU_CAMERA  3
#define DSRT_SIZEOF_POSE        4
#define DSRT_SIZEOF_FRAME       5
#define DSRT_SIZEOF_GBUFFER     6
#define DSRT_SIZEOF_RAYS        7
#define DSRT_SIZEOF_RAY_HITS    8
#define DSRT_SIZEOF_ACCUM       9
#define DSRT_SIZEOF_ADAPTIVE    10
#define DSRT_SIZEOF_ADAPTIVE_STATS 11
#define DSRT_SIZEOF_DENOISE_GUIDES 12
#define DSRT_SIZEOF_DENOISE     13
#define DSRT_SIZEOF_TEMPORAL    14
#define DSRT_SIZEOF_UPSCALE_GUIDES 15
#define DSRT_SIZEOF_UPSCALE     16
#define DSRT_SIZEOF_TEMPORAL_SHADING 19
#define DSRT_SIZEOF_BODY_MOTION 18   /* (17 is left unassigned and answers 0: tests/test_upscale_host.py holds it to that as the first unknown index of its day) */
#define DSRT_SIZEOF_COVERAGE_DESC 20
#define DSRT_SIZEOF_COVERAGE      21
#define DSRT_SIZEOF_COVERAGE_CLASSES 22
#define DSRT_SIZEOF_SENSOR        24   /* (23 is left unassigned and answers 0, like 17: tests/test_coverage_host.py holds it to that as the first unknown index of its day) */
#define DSRT_SIZEOF_STARS         26   /* (25 is left unassigned and answers 0, like 17 and 23: tests/test_sensor_host.py holds it to that) */
#define DSRT_SIZEOF_STARS_OUT     27
#define DSRT_SIZEOF_LENS          29   /* (28 is left unassigned and answers 0, like 17, 23 and 25: tests/test_stars_host.py holds it to that) */
#define DSRT_SIZEOF_LENS_OUT      30
size_t dsrt_sizeof(int which);

/* ===================================================================================== */
/* Host scene assembly -- no GPU involved.                                               */
/* Replaces the flattening half of build_gpu_scene (src/gpu_scene_builder.cpp:464-601):  */
/* collect_world :252-317, upsert_material :71-139, HostTextureRegistry :199-246,        */
/* build_bvh_for_triangles :343-459, and the OBJ/MTL loader inc/triangle_mesh.h:75-255.  */
/* ===================================================================================== */
typedef struct DsrtHostScene DsrtHostScene;

DsrtHostScene* dsrt_host_scene_create(void);
void           dsrt_host_scene_destroy(DsrtHostScene* hs);

/* Append the triangles of an OBJ file (with its MTL materials / map_Kd textures), exactly as
 * `world.add(make_shared<triangle_mesh>(path, lambertian(0.73), scale))` followed by the builder's
 * collect step would (src/main.cpp:238-245, src/gpu_scene_builder.cpp:259-283). */
int dsrt_host_scene_add_obj(DsrtHostScene* hs, const char* obj_path, double scale);

/* Append objects described in the small "world description" text format used by the tests and the
 * CLI (mat / sphere / tri / obj lines).  Objects are flattened in file order. */
int dsrt_host_scene_add_world_file(DsrtHostScene* hs, const char* world_path);

/* Append already-flattened primitives (reference layouts).  Material ids are rebased onto the
 * scene's material table. */
int dsrt_host_scene_add_arrays(DsrtHostScene* hs, const GPUTriangle* tris, int num_tris, const GPUSphere* spheres,
                               int num_spheres, const GPUMaterial* mats, int num_mats);

/* Decode an image file into the scene's texture pool the way the reference's builder does (HostTextureRegistry::get_or_load,
 * src/gpu_scene_builder.cpp:205-246: forced RGB, powf(c / 255, 2.2) per channel, one slot per distinct path, a file that cannot be
 * decoded becomes one white texel and is listed by dsrt_host_scene_texture_failures) and return its slot: the value a GPUTriangle's
 * albedo_tex must carry when triangles are added with dsrt_host_scene_add_arrays.  `flip_vertically` is the state of the reference's
 * global stb flag at that moment (image_texture::load sets it, inc/texture.h:133; SURVEY.md note T): 1 for any scene whose MTL named a map.
 * Returns the slot (>= 0) or a negative DSRT_ERR_*. */
int dsrt_host_scene_add_texture_file(DsrtHostScene* hs, const char* path, int flip_vertically);

/* Median-split BVH over all triangles added so far: leaf <= 4, std::nth_element on the centroid along
 * the widest centroid axis, pre-order node numbering (src/gpu_scene_builder.cpp:343-459). */
int dsrt_host_scene_build_bvh(DsrtHostScene* hs);

/* NOT the reference's tree: a binned surface-area-heuristic BVH in the same node format (leaf <= 4, pre-order), the
 * "non-parity fast mode" of SURVEY.md 8(f) n4.  Rays visit far fewer nodes; the frame is a statistically equivalent image
 * (ties between equal-distance hits and float grazing cases resolve differently), not the reference's bytes.  There is no
 * reference interface this replaces -- the reference has one builder (src/gpu_scene_builder.cpp:343-459). */
int dsrt_host_scene_build_bvh_sah(DsrtHostScene* hs);

/* NOT the reference's tree either: a linear BVH (Morton order + Karras' radix-tree construction) built ON THE GPU `device`, in the same
 * node format (leaf <= 4), copied into the host scene.  The "GPU-side BVH build" of SURVEY.md 8(f) n4: milliseconds instead of the
 * seconds of the host builders, for hosts that rebuild per frame as the reference does (src/main.cpp:405).  Same parity status as the
 * SAH tree: a statistically equivalent image, exact agreement between the kernel and the oracle on this tree.  `build_ms` (optional)
 * receives the device time of the construction kernels, `total_ms` the whole call including the triangle upload and the copy back.
 * The tree is deterministic, bit for bit: a pure function of the triangles (contract: the header comment of csrc/bvh_lbvh.hip). */
int dsrt_host_scene_build_bvh_gpu(DsrtHostScene* hs, int device, float* build_ms, float* total_ms);

/* Fill `out` with HOST pointers into the scene's arrays (valid until the scene is modified or
 * destroyed).  Camera / params / sun fields of `out` are zeroed; set them with dsrt_scene_set_frame. */
int dsrt_host_scene_view(const DsrtHostScene* hs, GPUScene* out);

/* Textures that could not be decoded while objects were added.  Like the reference (stbi_load failure, src/gpu_scene_builder.cpp:216-221)
 * the builder goes on with a 1x1 white texel for such a map and prints a warning -- but the reference's stb_image also decodes BMP,
 * TGA, GIF, PSD, HDR, PIC, interlaced PNG and CMYK JPEG, while this library decodes PNM, non-interlaced PNG and 1- or 3-component JPEG only.  A scene for which this returns
 * non-zero therefore does NOT render like the reference would; hosts that care should refuse it (dsrt_render --strict-textures does,
 * bench.py labels the run).  Returns the number of failed maps; if `names` is given, their paths, newline-separated, as far as `cap` allows. */
int dsrt_host_scene_texture_failures(const DsrtHostScene* hs, char* names, size_t cap);

/* Greatest number of entries the reference traversal's stack can hold for this BVH (= height - 1). */
int dsrt_host_scene_bvh_stack_need(const DsrtHostScene* hs);

/* Defaults of build_gpu_scene for everything that is not geometry (src/gpu_scene_builder.cpp:560-598):
 * camera, params {gamma 2, exposure 50, use_bvh 1, rng_mode 0, tile_size 0}, black sky, seed 1337,
 * sun enabled with radiance (1e5, 9.5e4, 9e4). */
void dsrt_scene_set_frame(GPUScene* scene, const GPUCamera* cam, const float sun_dir_model[3]);

/* ===================================================================================== */
/* Pose file and camera -- src/main.cpp:139-173 (reader), :310-357 (world->model), :178-187 and
 * inc/camera.h:91-133 (camera).                                                          */
/* ===================================================================================== */
typedef struct DsrtPose {
    double cam_pos_world[3];
    double model_pos_world[3];
    float  model_euler_deg[3];      /* yaw, pitch, roll -- stored as float like PoseEntry, main.cpp:95-99 */
} DsrtPose;

typedef struct DsrtFrame {
    float  cam_in_model[3];
    float  sun_dir_model[3];
    double sep_m;
    int    skipped;                 /* sep_m < 1.0: the reference skips the frame, main.cpp:342-345 */
} DsrtFrame;

/* Reads up to `cap` poses; *count receives the number of valid lines in the file (may exceed cap).
 * Returns DSRT_ERR_IO if the file cannot be opened or holds no valid pose (read_pose_file returns false). */
int dsrt_read_pose_file(const char* path, DsrtPose* out, int cap, int* count);
int dsrt_pose_to_frame(const DsrtPose* pose, DsrtFrame* out);
/* World-frame points / directions of a pose's epoch (doubles, as the pose file has them) into the model frame that GPUScene lives in, for the ray queries
 * (dsrt_trace_rays).  Points: yaw_about_y(p - model_pos_world, -yaw) in double, then narrowed to float -- exactly the operations dsrt_pose_to_frame applies to
 * the camera, so dsrt_pose_points_to_model(cam_pos_world) == cam_in_model bit for bit.  Directions: yaw_about_y(d, -yaw), not normalised.
 * `world_xyz` and `model_xyz` hold n x 3 values; DSRT_ERR_INVALID for a NULL pose, n < 0, or NULL arrays with n > 0. */
int dsrt_pose_points_to_model(const DsrtPose* pose, int n, const double* world_xyz, float* model_xyz);
int dsrt_pose_dirs_to_model(const DsrtPose* pose, int n, const double* world_xyz, float* model_xyz);
/* point_camera_at + camera::initialize + toGPUCamera: vup (0,1,0), aperture 0, focus = |from - at|. */
int dsrt_camera_look_at(GPUCamera* out, const float from[3], const float at[3], float vfov_deg, int width, int height,
                        int spp, int max_depth);

/* Decode a texture file exactly as the scene builder does (PNM, non-interlaced PNG, baseline / progressive JPEG; forced to 3 channels like the
 * reference's stbi_load(..., 3), src/gpu_scene_builder.cpp:215; `flip_vertically` as stbi_set_flip_vertically_on_load).  Pass rgb = NULL to ask
 * for the size only.  DSRT_ERR_IO if the file cannot be read or is in a format this library does not decode. */
int dsrt_decode_image_file(const char* path, int flip_vertically, int* width, int* height, uint8_t* rgb, size_t cap);

/* P6 writer, as the tail of gpu_render_scene (src/gpu_render.cu:1099-1107). */
int dsrt_write_ppm(const char* path, const uint8_t* rgb, int width, int height);
/* 8-bit RGB PNG: what the reference obtains by shelling out to ImageMagick on the PPM (src/main.cpp:28-36). */
int dsrt_write_png(const char* path, const uint8_t* rgb, int width, int height);
/* Portable float map: `channels` 1 ("Pf") or 3 ("PF") floats per pixel, `data` in image order (top row first, as every buffer of this
 * library); the file holds the rows bottom-up, as the format wants, little-endian (scale -1).  For the G-buffer channels (dsrt_render_gbuffer). */
int dsrt_write_pfm(const char* path, const float* data, int width, int height, int channels);

/* ===================================================================================== */
/* Device side.                                                                          */
/* ===================================================================================== */
typedef struct DsrtContext DsrtContext;

/* The first call of either of these two sets the environment variable GPU_MAX_HW_QUEUES to 16 if the host has not set it (frames in flight
 * on separate streams only overlap on the device if each stream has a hardware queue of its own, and the HIP runtime reads the variable
 * when it initialises): a host that minds sets the variable itself, or initialises HIP, before calling.  Loading the library changes nothing. */
int  dsrt_device_count(void);
int  dsrt_ctx_create(int device, DsrtContext** out);
void dsrt_ctx_destroy(DsrtContext* ctx);

/* A second context on the same device that SHARES `src`'s resident scene (no copy, no re-upload) and has its own camera / sun
 * and its own working buffers: what a host needs to keep several frames of one scene in flight on separate streams.  A context
 * serves one render at a time (a second dsrt_render on it waits for the first, on any stream).  Uploading a new scene into
 * either context afterwards does not affect the other.  No reference counterpart (the reference renders one frame at a time). */
int  dsrt_ctx_clone(const DsrtContext* src, DsrtContext** out);
int  dsrt_ctx_device(const DsrtContext* ctx);

/* THE CERTIFIED SECOND TREE (round 4).  The reference's answer to a BVH query depends on its own median-split tree only in three narrow ways: triangles under
 * a zero-thickness box are never reached (src/gpu_render.cu:312), of two accepted triangles at exactly the same t the one tested later wins (:353), and a hit
 * computed in front of its own leaf box's entry distance is found or not depending on what was found before.  Everywhere else the answer is simply the accepted
 * triangle of smallest t -- whatever tree found it.  With this option the next dsrt_scene_upload also builds a binned-SAH tree over the reachable triangles
 * (boxes widened by 2^-16 of the scene's extent); a ray walks THAT tree (a third fewer node visits on a mesh of long thin members), the kernel then checks the
 * three conditions exactly -- no tie, the hit inside its REFERENCE-leaf box's slab interval as the reference's own arithmetic computes it, no zero direction
 * component -- and any ray that fails one is walked again on the reference tree (a handful per million).  The image is the reference's, byte for byte, provided
 * Moller-Trumbore's computed t of every accepted triangle is accurate to 2^-10 relative (the margin by which the second tree's distance culling is relaxed;
 * a wider margin costs 2 % per factor 16): what could slip through is a triangle hit at a grazing angle below ~3e-4 rad whose computed t lands IN FRONT of a nearer
 * triangle the second walk has already found -- the reference would then show the farther triangle, the second tree the nearer one; estimated at well under one ray
 * per 1080p x 1000-sample frame, observed in none (the headline frame in both math modes: 7.4e9 rays).  tests/test_gpu_certified_tree.py compares whole frames,
 * the headline frame included, with the reference kernel's own images, and DsrtRenderDesc.collect_counters = 3 AUDITS a launch: every answer of the second tree
 * is also walked on the reference tree and compared (DsrtStats.certificate_audit_mismatches), for a host that wants the check on its own mesh.  Scenes with
 * spheres reaching beyond 30 extents of the mesh, and cameras farther than that, use the reference tree only.  Off by default; the
 * environment variable DSRT_CERTIFIED_TREE=1 switches it on for contexts created afterwards (the drop-in gpu_render_scene included).  Costs one more tree in HBM
 * (about as much again as the scene) and the SAH build at upload (0.2 s per million triangles).  DSRT_TUNE_REFERENCE_WALK renders without it. */
int  dsrt_ctx_set_certified_tree(DsrtContext* ctx, int on);
int  dsrt_ctx_has_certified_tree(const DsrtContext* ctx);
/* Test hook, no GPU involved: what the upload would prepare for the certified second tree of this host scene (which must carry the reference's tree).
 * counts = {triangles, triangles the reference tree can never reach, triangles in the second tree, its nodes, its height, 1 if no sphere is too far away};
 * *pad = the widening of its boxes; the arrays (each may be NULL) receive the per-triangle flags and reference-leaf boxes and the tree itself. */
int  dsrt_host_scene_second_tree_probe(const DsrtHostScene* hs, int counts[6], float* pad, uint8_t* unreachable, float* leaf_box, GPUBVHNode* nodes, int max_nodes,
                                       int* order, int max_order);
int  dsrt_dropin_has_certified_tree(void);     /* the same question about the scene the drop-in gpu_render_scene converted last (it looks at DSRT_CERTIFIED_TREE on every call) */

/* Upload + re-layout for the GPU (once per scene, not per frame).  `scene` holds HOST pointers in the
 * reference layouts (as from dsrt_host_scene_view); its camera/params/sun are recorded as the current frame.
 * Replaces the upload half of build_gpu_scene (src/gpu_scene_builder.cpp:322-331, 475-546). */
int dsrt_scene_upload(DsrtContext* ctx, const GPUScene* scene);
/* Same, for a GPUScene whose array members are DEVICE pointers (what the reference's own builder
 * produces and what gpu_render_scene receives, src/gpu_render.cu:1037-1066). */
int dsrt_scene_upload_device(DsrtContext* ctx, const GPUScene* scene);
/* Per-frame update: only camera and sun change between frames (src/main.cpp:399-405). */
int dsrt_scene_set_camera_sun(DsrtContext* ctx, const GPUCamera* cam, const float sun_dir_model[3]);

/* ===================================================================================== */
/* MOVABLE RIGID BODIES -- a static part and up to 15 bodies whose poses are set per frame ON THE DEVICE.  No reference counterpart: the reference renders one
 * rigid mesh in the model frame (a second vehicle, a rotating array or a tumbling target means re-flattening, re-building and re-uploading everything there and,
 * before this, here).  Like the SAH and LBVH trees the bodies tree is NOT the reference's tree; its standing is theirs: the kernels agree exactly with the CPU
 * oracle on the same tree.  No render, G-buffer or ray-query kernel knows about bodies: they read the resident scene, and the resident scene moves.
 *
 * THE TREE.  One tree in the ordinary node format, fixed topology.  Every non-empty body has a median-split subtree over its own triangles (the builder of
 * dsrt_host_scene_build_bvh: leaf <= 4, a leaf of any size where the centroids coincide); the subtrees hang from a chain of top nodes in body order,
 * T0 = (body_a, T1), T1 = (body_b, T2), ..., last = (body_y, body_z), empty bodies left out, no top node at all with one non-empty body.  Nodes are numbered
 * in pre-order, tri_indices is global.  A rigid motion keeps a subtree's topology good; only boxes change (an axis-aligned box does not rotate).
 *
 * THE ARITHMETIC of a pose update -- fp32, every operation one correctly rounded operation, never contracted, in the order written; the host form, the device
 * form and tests/_bodies_model.py agree bit for bit.  That word-for-word equality holds while every posed coordinate is finite (a finite pose can still overflow
 * a large coordinate; the NaN that follows differs in its sign bit between host and device):
 *   pose          12 floats, row-major  r00 r01 r02 tx | r10 r11 r12 ty | r20 r21 r22 tz,  in the model frame
 *   point         x' = ((r00*x + r01*y) + r02*z) + tx,  y' and z' likewise with rows 1 and 2
 *   normal        the same without the translation; NOT renormalised (an orthonormal R is the caller's business)
 *   source        always the REST pose (the triangles as they were when the bodies tree was built), never the previous pose: no drift accumulates
 *   pair record   v0', v1' - v0', v2' - v0'  (what the upload forms from any triangle)
 *   leaf box      per axis lo = fminf, hi = fmaxf over the leaf's triangles' nine transformed coordinates; then lo = lo + 0.0f, hi = hi + 0.0f (a -0 that fminf
 *                 may or may not return becomes +0 either way); then, if hi == lo:  lo = lo - pad, hi = hi + pad,  with the BODY's pad =
 *                 extent > 0 ? extent * (1 / 4096) : 1e-6, extent = largest edge of the body's unpadded root box at rest
 *   internal box  fminf / fmaxf of the two children's boxes; a body's root box is that of its root node; the chain's boxes are formed the same way
 *   ordering sums lo.x + hi.x of a child box, in float
 *   body 0        never moves; its boxes are computed once, at build, by the same rule
 * ===================================================================================== */
#define DSRT_MAX_BODIES 16
/* Start a new body and return its index (1 .. 15).  Triangles added afterwards (dsrt_host_scene_add_obj, _add_arrays, _add_world_file) belong to it; triangles
 * added before the first call are body 0, the static part.  Spheres, materials and textures stay global and static. */
int dsrt_host_scene_begin_body(DsrtHostScene* hs);
int dsrt_host_scene_body_count(const DsrtHostScene* hs);                                      /* 1 for a scene that never began a body */
int dsrt_host_scene_body_range(const DsrtHostScene* hs, int body, int* first_tri, int* num_tris);
/* Build the bodies tree (above) and keep the rest-pose copy of the movable bodies' vertices and normals and one pad per body.  The other three builders keep
 * working on a scene with bodies: they treat it as one flat static scene (and dsrt_host_scene_set_body_poses then refuses it). */
int dsrt_host_scene_build_bvh_bodies(DsrtHostScene* hs);
/* The CPU statement of the device update: bodies first_body .. first_body + count - 1 take the poses given (12 floats each), applied to the rest pose.
 * Afterwards dsrt_host_scene_view is an ordinary GPUScene of the posed scene: the oracle can render it and dsrt_scene_upload can pack it.  DSRT_ERR_INVALID for a
 * body outside 1 .. body_count - 1, a pose entry that is not finite, or a scene whose tree is not the bodies tree; a refused call changes nothing. */
int dsrt_host_scene_set_body_poses(DsrtHostScene* hs, int first_body, int count, const float* poses);

/* Upload `hs` (which must carry the bodies tree) exactly as dsrt_scene_upload packs its view -- the same bytes in the same arrays; `frame` supplies only camera,
 * params and Sun -- and keep resident what a pose update needs: the rest-pose records, the list of movable pair records, per depth the internal node records of
 * the movable subtrees, the chain and the pads (layout: DESIGN.md).  The certified second tree is never built for such a scene (dsrt_ctx_has_certified_tree
 * returns 0 whatever dsrt_ctx_set_certified_tree asked for). */
int dsrt_scene_upload_bodies(DsrtContext* ctx, const DsrtHostScene* hs, const GPUScene* frame);
/* Pose bodies first_body .. first_body + count - 1 of the resident scene: `poses` is a HOST array of 12 * count floats.  On `stream`, after the context's last
 * launch: one transform launch over the moved bodies' pair records (triangles, normals, a box per pair record), one refit launch per tree depth, deepest first,
 * one small launch for the chain and the scene's root box; then the 24-byte root box is read back, so that the pre-pass cull, the distance checks of a render and
 * dsrt_ctx_scene_bounds see the posed scene -- THE CALL IS THEREFORE SYNCHRONOUS.  No atomics and no waiting between workgroups: the result is deterministic, and
 * equal word for word to dsrt_host_scene_set_body_poses followed by dsrt_scene_upload.  `ms` (optional) receives the device time of the launches: measured
 * 0.05 / 0.07 / 0.12 ms for a body of 10^4 / 10^5 / 10^6 triangles beside a 10^6-triangle static part on an MI355X, against 98 / 111 / 283 ms
 * for host posing + dsrt_host_scene_build_bvh_gpu + dsrt_scene_upload.
 * The resident scene is shared with the context's clones (dsrt_ctx_clone): they see the new poses, and the caller must have NO LAUNCH OF A CLONE IN FLIGHT during
 * this call.  The convenience temporal sequence of the calling context (dsrt_render_denoised_temporal_to_host) starts afresh: its history assumes a static scene -- unless
 * dsrt_ctx_set_temporal_bodies is on for it (TEMPORAL ACCUMULATION WITH BODIES below).
 * A dsrt_render_batch launch has one scene and therefore one set of poses: a sequence with moving bodies renders one launch per frame.
 * Refusals: those of the host form, DSRT_ERR_NO_SCENE, and DSRT_ERR_INVALID when the resident scene has no bodies; a refused call touches no buffer. */
int dsrt_scene_set_body_poses(DsrtContext* ctx, int first_body, int count, const float* poses, void* stream, float* ms);
int dsrt_ctx_body_count(const DsrtContext* ctx);                                              /* bodies of the resident scene; 0 = not uploaded with dsrt_scene_upload_bodies */
/* Device times of the three stages of the context's last dsrt_scene_set_body_poses that was given `ms`: transform, refit (all depths), chain + root box. */
int dsrt_ctx_body_update_ms(const DsrtContext* ctx, float ms[3]);

/* PARITY DOMAIN.  rng_mode 0 renders the reference's bytes (as the chosen math_mode defines them) for scenes whose coordinates keep the reference's own
 * intermediates out of the subnormal and overflow ranges: for every box centre c, ray origin o and direction d the walk meets, |c - o| * |d| is zero or lies
 * in [2^-100, 2^100] (metres-scale scenes are 20 orders of magnitude inside; tested from 1e-15 to 1e9 times the station's size, tests/test_gpu_parity.py
 * ::test_scaled_scenes_match_the_oracle_bit_for_bit).  The kernel orders a node's children by 2 d where the reference compares d (render_kernel.hip): the
 * same comparison exactly when no intermediate is subnormal or overflows.  Outside that range images are still valid renders, but near/far ties may
 * resolve differently from the reference's. */
typedef struct DsrtRenderDesc {
    int      width, height;         /* gpu_render_scene(scene, width, height)                     */
    int      spp;                   /* <1 -> 1, as src/gpu_render.cu:987-988                      */
    int      max_depth;             /* <=0 -> 12, as :723-725                                     */
    float    gamma;                 /* <=0 -> 1, as :1043                                         */
    uint64_t seed;
    int      rng_mode;              /* 0 = reference LCG stream per pixel (parity mode, bit-exact);
                                       1 = rocRAND Philox4x32-10, one sub-sequence per (pixel, sample): samples become
                                           independent work items (statistically equivalent image, not bit-identical to mode 0);
                                           a pixel's samples are summed as integers in units of 2^-20, so the image is a function
                                           of (scene, camera, seed) alone -- not of sharding, scheduling or which lane drew what.
                                       Mode 1, exactly (restated on the CPU by oracle/dsrt_oracle.c, dsrt_oracle_render_rect; tests/test_gpu_rng_mode1.py):
                                         - key: `seed`, low 32-bit word first (key = {seed & 0xFFFFFFFF, seed >> 32});
                                         - pixel (x, y), sample k (0 <= k < spp) draws from sub-sequence (x + y*W)*spp + k, a 64-bit number, with y = 0 the
                                           BOTTOM row as in mode 0 (the kernel's y; the image stores that pixel in row H-1-y);
                                         - draw n of a sample (n counted from 0 at the start of every sample) is word n & 3 of the Philox4x32-10 block with
                                           counter {n >> 2, 0, sub & 0xFFFFFFFF, sub >> 32}: rocrand_init(seed, sub, 0) followed by n + 1 calls of rocrand();
                                         - a draw maps to [0,1) as (word & 0xFFFFFF) / 2^24; the draws are consumed in mode 0's order (jitter x, jitter y,
                                           then ray_color's);
                                         - each sample's value: the sample's colour clamped to [0,1] (as mode 0), then (uint32_t)(c * 2^20 + 0.5f) in fp32;
                                         - a pixel's sum over its spp samples is a 64-bit integer per channel;
                                         - its mean is (float)((double)sum * (1.0 / 2^20 / spp)), computed in double and converted to float once;
                                         - the tone map and the 8-bit store are mode 0's (clamp to [0,10], pow(1/gamma), clamp to [0,1], 255.99 * c);
                                         - pixels of culled tiles are black (all-zero bytes and +0.0f), which is what they render to anyway.
                                       SAMPLE SETS (dsrt_render_accumulate below): sample k of a pixel is defined by (seed, pixel, spp, k) alone -- sub-sequence
                                       (x + y*W)*spp + k, jitter (k + r)/spp with spp the PLANNED count -- so it does not matter which launch draws it.  A launch
                                       with (first, count, stride) renders, for every pixel, the set {first + j*stride : 0 <= j < count} of a frame planned at spp
                                       samples and ADDS its sums to the caller's; the sums over disjoint sets add up to the sum over their union, exactly, and
                                       resolved at samples_done = spp the union of sets that cover [0, spp) is dsrt_render's image byte for byte.
                                         - a partial set is a valid image, stratified differently: the jitter keeps sample k in the k-th strip of its pixel, so a
                                           contiguous [0, n) covers only part of every pixel.  Interleaved passes (first = p, stride = P, p = 0 .. P-1) are the form
                                           for previews: after pass p every pixel has samples spread over its whole area;
                                         - second moment (optional): per sample and channel, with q the quantised value above, sq = (uint32_t)(((uint64_t)q*q + 2^19) >> 20),
                                           the squared clamped sample in units of 2^-20, rounded; summed as a 64-bit integer like q;
                                         - resolve with n = samples_done: the mean, tone map and bytes are the ones above with spp replaced by n; the variance of the
                                           mean, per pixel and channel, in double and in exactly this order (correctly rounded operations only, no sqrt):
                                             s = (double)S * 2^-20;  s2 = (double)S2 * 2^-20;  v = (s2 - s * s / n) / (n - 1);  v = v > 0 ? v : 0;  out = (float)(v / n) */
    int      tile_size;             /* screen-tile edge in pixels, multiple of 8; 0 -> 8          */
    int      shard_rank;            /* this process renders tiles t with t % shard_count == shard_rank */
    int      shard_count;           /* 0 or 1 -> whole image                                      */
    int      collect_counters;      /* 1 -> counting build of the kernel (fills DsrtStats); 2 -> counting build WITHOUT the any-hit
                                       shadow-ray early-out, whose counters equal the reference traversal's exactly; 3 -> counting build
                                       with the CERTIFICATE AUDIT: when the certified second tree is in use, every one of its answers is also walked
                                       on the reference tree and compared (DsrtStats.certificate_audited / certificate_audit_mismatches) */
    int      checked;               /* 1 -> bounds-checked build of the kernel (tests / first runs) */
    int      stack_entries;         /* LDS short-stack entries per lane: 0 or 8 (the only size built)  */
    int      tune[4];               /* scheduling knobs, 0 = default: {min_walk_iters, advance_budget, leaf_ratio4, flags}.  None of them
                                       changes a pixel (tested against the oracle in every combination).  Flags, DSRT_TUNE_* below: the low
                                       two bits choose the pre-pass, the others switch one scheduling measure off each.  Any other bit is
                                       refused (DSRT_ERR_INVALID): development switches are not part of a render's description -- see
                                       dsrt_dev_set_experiment below */
    int      math_mode;             /* where sinf / cosf / powf come from -- the three library functions of the path (src/gpu_render.cu:104-106, 157-158, 211,
                                       1019-1021).  0 (default): include/dsrt_detmath.h, built from correctly rounded operations only and shared with the CPU
                                       oracle: the image is a function of the inputs alone, the same on the GPU and on a CPU, and what every parity test
                                       against the oracle uses.  1: the device math library's own (what the reference's source gets when hipcc compiles it
                                       for this GPU WITH FLOATING-POINT CONTRACTION OFF): the image is then, byte for byte, the one the reference's own kernel
                                       renders on the same GPU when built that way (oracle/_ref/ref_gpu: hipify-perl + hipcc -ffp-contract=off;
                                       tests/golden/ref_gpu_images.json, tests/test_gpu_reference_fixtures.py).  hipcc's and nvcc's DEFAULT builds contract
                                       a * b + c into one rounding; against such a build (or libdevice's math) either mode is a statistical match only
                                       (oracle/_ref/ref_gpu_fma).  Mode 0 has the same standing against the reference's kernel built with dsrt_detmath.h in
                                       place of those three functions (oracle/_ref/ref_gpu_detmath, tests/golden/ref_gpu_detmath_images.json).  The two modes differ in the last place of those three
                                       functions and therefore, one LCG stream per pixel being what it is, in individual pixels; statistically they are
                                       the same picture.  rng_mode and math_mode are independent */
} DsrtRenderDesc;

#define DSRT_TUNE_NATURAL_ORDER   1    /* tiles in natural order, no empty-tile culling (no pre-pass at all)                   */
#define DSRT_TUNE_NO_CULLING      2    /* costliest-first order, but no tile is dropped as provably empty                     */
#define DSRT_TUNE_NO_HELPERS      4    /* idle lanes do not trace shadow rays for busy lanes of their wave                    */
#define DSRT_TUNE_NO_PROBE        8    /* no probe launch to refine the tile order (rng_mode 0)                               */
#define DSRT_TUNE_NO_STEALING    16    /* rng_mode 1: idle lanes do not take over samples of busy lanes                       */
#define DSRT_TUNE_NO_PRIORITY    32    /* rng_mode 0: waves holding a heavy tile's pixel do not raise their issue priority    */
#define DSRT_TUNE_REFERENCE_WALK 64    /* every ray walks the reference tree even when the certified second tree is resident   */
#define DSRT_TUNE_FLAG_MASK      127

typedef struct DsrtStats {
    float    kernel_ms;             /* HIP events around the render kernel on the given stream (0 if timing off) */
    int      waves_launched;
    uint32_t device_flags;          /* checked-mode status word (0 = clean)                       */
    int      lds_stack_entries;
    uint64_t samples, rays, primary_hits, box_fetches, nodes_entered, internal_entered, tri_tests, hit_updates,
             sphere_tests, shaded_hits, tex_fetches, stack_spills, max_stack;
    /* lane-slot accounting of the counting build: every lane of a wave adds 1 per wave iteration of the node loop / the
     * triangle loop / the advance loop, so active / slots is the SIMD utilisation of that loop */
    uint64_t node_slots, tri_slots, adv_slots, adv_active;
    /* where the idle lanes of the node loop were: parked at a leaf / waiting for their state machine / out of work */
    uint64_t idle_at_leaf, idle_waiting, idle_done;
    /* node visits at BVH depth < 6 / 9 / 12 (root = 0) */
    uint64_t visits_depth_lt6, visits_depth_lt9, visits_depth_lt12;
    /* tiles of this shard / tiles the pre-pass proved empty and left out (their pixels are exactly black) */
    uint64_t tiles_total, tiles_culled;
    /* counting build: sum over the waves of the time each spent in the kernel, in ticks of the 100 MHz wall clock; divided by
     * (waves_launched x kernel time) it is the fraction of the launch the average wave was resident */
    uint64_t wave_ticks;
    /* counting build, certified second tree in use: BVH queries whose certificate failed and which were walked again on the reference tree */
    uint64_t certificate_fallbacks;
    /* collect_counters = 3 (the CERTIFICATE AUDIT): answers of the second tree that were also walked on the reference tree, and how many of them differed (must be 0) */
    uint64_t certificate_audited, certificate_audit_mismatches;
    /* counting build, ms after the first wave started: the heavy / the light work queue handed out its last item, the last wave left */
    float    heavy_queue_empty_ms, light_queue_empty_ms, last_wave_exit_ms;
    int      certified_tree_used;   /* 1: the rays of this launch started on the certified second tree (dsrt_ctx_set_certified_tree) */
} DsrtStats;

/* Number of bytes of the compact per-shard output of dsrt_render for this desc (rgb8) and the number of
 * tiles this shard owns / the padded per-shard tile count (equal on every rank, for a gather). */
int dsrt_shard_layout(const DsrtRenderDesc* desc, int* tiles_total, int* tiles_this_shard, int* tiles_per_shard_padded,
                      size_t* rgb8_bytes_padded);

/*
 * Render.  Asynchronous on `stream` (a hipStream_t passed as void*; NULL = the null stream) unless
 * `stats` is non-NULL, in which case the call synchronises the stream and fills `stats`.
 *   d_rgb8 : DEVICE buffer.  shard_count <= 1: width*height*3 bytes in image order (top row first), what
 *            the reference copies back and writes after the P6 header (src/gpu_render.cu:1087-1106).
 *            shard_count  > 1: tiles_per_shard_padded * tile*tile*3 bytes, tile-major, local tile k =
 *            global tile k*shard_count + shard_rank, rows of a tile top first.
 *   d_f32  : optional DEVICE buffer, same indexing, 3 floats per pixel: the value multiplied by 255.99
 *            (:1028), for the L-infinity parity check.  May be NULL.
 */
/* Bounding box of the resident scene's BVH root (all zeros without a BVH). */
int dsrt_ctx_scene_bounds(const DsrtContext* ctx, float lo[3], float hi[3]);

int dsrt_render(DsrtContext* ctx, const DsrtRenderDesc* desc, uint8_t* d_rgb8, float* d_f32, void* stream, DsrtStats* stats);

/*
 * Render `frames` views of the resident scene as ONE launch: the reference's frame loop (src/main.cpp:310-431) with the scene kept and
 * only camera and sun changing, but with all frames' pixels in a single pool of work.  In rng_mode 0 a pixel is a serial chain of spp
 * samples and a frame rendered alone ends in a tail of a few such chains on an otherwise empty chip; here a lane that finishes a pixel
 * of frame f goes straight on to frame f + 1, so the chains of one frame run under the bulk of the next ones.  Every frame's image is the
 * image dsrt_render gives for that camera and sun, byte for byte (rng_mode 0: the reference's; rng_mode 1: seed-determined).
 *   cameras      : `frames` cameras (dsrt_camera_look_at / dsrt_pose_frame_camera), HOST array
 *   sun_dirs_xyz : 3 * frames floats, HOST array (radiance and the enabled flag are the context's, dsrt_scene_set_camera_sun)
 *   d_rgb8       : DEVICE buffer, frames * width*height*3 bytes: the images one after another, each in dsrt_render's layout
 *   d_f32        : optional DEVICE buffer, frames * width*height*3 floats
 * With shard_count > 1 every frame's part is this rank's compact tile buffer (dsrt_shard_layout: rgb8_bytes_padded each), i.e. a rank renders its
 * tiles of ALL the frames as one pool -- the split that scales a sequence over the GPUs of a node in either rng_mode, one gather for the lot.
 * Work is handed out frame after frame in the order given (put the costliest -- nearest -- frames first), every frame's first eighth of heavy tiles
 * before any frame's remainder; in rng_mode 0 at 256 samples and more each frame's tiles are first re-sorted by a probe launch, as in dsrt_render.
 * Production kernel only (no counters, not `checked`); frames * pixels per frame (x 16 in rng_mode 1) must stay below 2^32 -- split a longer
 * sequence into several calls.  Asynchronous on `stream` unless `stats` is given
 * (kernel_ms then covers the one launch; the per-frame pre-passes before it are not included).
 */
int dsrt_render_batch(DsrtContext* ctx, const DsrtRenderDesc* desc, int frames, const GPUCamera* cameras, const float* sun_dirs_xyz,
                      uint8_t* d_rgb8, float* d_f32, void* stream, DsrtStats* stats);
/* The same with the images delivered to HOST memory (frames * width*height*3 bytes), synchronously: for hosts without device code of their own,
 * like the reference's main.cpp. */
int dsrt_render_batch_to_host(DsrtContext* ctx, const DsrtRenderDesc* desc, int frames, const GPUCamera* cameras, const float* sun_dirs_xyz,
                              uint8_t* h_rgb8, DsrtStats* stats);

/*
 * GROUND-TRUTH G-BUFFER.  One primary ray per pixel through the pixel CENTRE -- the reference's camera ray (make_camera_ray_jittered, src/gpu_render.cu:941-968)
 * with jx = jy = 0.5 -- for the context's current camera and sun (dsrt_scene_set_camera_sun), and per pixel what its first hit is.  The hit is the reference's
 * own primary query, scene_hit(ray, 0.001f, 1e9f) (:744), on the REFERENCE tree even when the certified second tree is resident: bit for bit the triangle,
 * t, u, v the oracle's scene_hit returns (ties resolve by the reference's visit order).  Pixels in the rgb8 output's order: top row first, so buffer row r
 * is camera row H-1-r.  Every channel is optional (NULL = not written); each is a DEVICE buffer of width*height elements of the type and count below.
 *
 *   channel      type x comps  on a hit                                                                        on a miss
 *   t            f32 x 1       ray parameter of the hit                                                        +inf
 *   range        f32 x 1       t * sqrtf(dot(d, d)), f32 ops in that order: Euclidean distance, model units    +inf
 *   depth        f32 x 1       t * dot(d, -camera.w): distance along the optical axis                          +inf
 *   position     f32 x 3       p = o + t d as ray_at forms it (model frame)                                     0
 *   normal       f32 x 3       the hit record's normal: interpolated, normalised, face-forwarded (set_face_normal) 0
 *   uv           f32 x 2       barycentric u, v of the hit (0, 0 for spheres)                                  0
 *   albedo       f32 x 3       material albedo x tex2D texel at the interpolated uv, as ray_color forms it (:763-774) 0
 *   prim_id      i32           original triangle index (into GPUScene.triangles); sphere s -> -2 - s           -1
 *   material_id  i32           the hit record's material id                                                     -1
 *   sun_cos      f32 x 1       fmaxf(0, dot(normal, normalize(-sun_dir))); 0 when the sun is disabled          0
 *   flags        u8            DSRT_GB_* below                                                                  0
 *
 * DSRT_GB_SUN_VISIBLE: sun_cos > 0 and the reference's shadow ray (origin p + normal * 1e-3f, direction normalize(-sun_dir), scene_hit(..., 0.001f, 1e9f); :800-810)
 * is not blocked -- set for every hit whatever its material: a geometric shadow mask.  The shadow rays are traced only when `flags` is asked for.
 * No sinf / cosf / powf are involved: DsrtRenderDesc.math_mode does not matter.
 */
typedef struct DsrtGBuffer {
    float*   t;
    float*   range;
    float*   depth;
    float*   position;
    float*   normal;
    float*   uv;
    float*   albedo;
    int32_t* prim_id;
    int32_t* material_id;
    float*   sun_cos;
    uint8_t* flags;
} DsrtGBuffer;

#define DSRT_GB_HIT          1    /* the primary ray hit something                  */
#define DSRT_GB_FRONT_FACE   2    /* ... on the side its (outward) normal faces      */
#define DSRT_GB_SPHERE       4    /* ... and that something is a sphere              */
#define DSRT_GB_SUN_VISIBLE  8    /* the hit point sees the Sun (see above)          */

/* The G-buffer of the current camera into the DEVICE buffers of `gb`.  Uses desc->width / height only (the sampling fields are ignored).
 * DSRT_ERR_INVALID: width or height < 2 (the camera divides by W-1 and H-1), shard_count > 1, a NULL desc or gb; DSRT_ERR_NO_SCENE before an upload.
 * Asynchronous on `stream` unless `stats` is given; then the call synchronises and fills kernel_ms, waves_launched and device_flags (the rest is 0).
 * The context's camera, sun, scene and working buffers are left as they were: a render after this call gives the same bytes as one before it.
 * Like a render, the call waits for the context's previous render, and the next render waits for it. */
int dsrt_render_gbuffer(DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtGBuffer* gb, void* stream, DsrtStats* stats);
/* The same into HOST buffers (each channel of `gb` a host pointer or NULL), synchronously. */
int dsrt_render_gbuffer_to_host(DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtGBuffer* gb, DsrtStats* stats);

/*
 * COVERAGE.  Sub-pixel ground truth: n primary rays per pixel instead of one, and per pixel how many of them hit (a soft mask), which (a bit mask), how many of
 * the hits see the Sun (an antialiased shadow mask), how many fall into each of up to 16 triangle ranges (per-body soft masks), and the whole G-buffer record of
 * one REPRESENTATIVE hit.  Camera, sun, tree and hit are the G-BUFFER's: the context's current camera and sun, scene_hit(ray, 0.001f, 1e9f) on the REFERENCE tree.
 * No reference counterpart.  No sinf / cosf / powf: DsrtRenderDesc.math_mode does not matter.
 *
 * THE ARITHMETIC.  fp32; every operation one correctly rounded IEEE operation, never contracted, in the order written.
 *   Sub-samples, DsrtCoverageDesc {pattern, samples}:
 *     DSRT_COVERAGE_GRID (0)      samples = S in 1..8, n = S*S;  sub-sample k = j*S + i (0 <= i, j < S):
 *                                   jx = ((float)i + 0.5f) / (float)S;   jy = ((float)j + 0.5f) / (float)S        -- measures the covered AREA of the pixel
 *     DSRT_COVERAGE_DIAGONAL (1)  samples = n in 1..64;  sub-sample k:
 *                                   jx = jy = ((float)k + 0.5f) / (float)n                                          -- measures the covered share of the pixel's DIAGONAL,
 *                                   which is what a render converges to: the renderer takes jx and jy of sample k both from stratum k (src/gpu_render.cu:995-996)
 *     anything else is DSRT_ERR_INVALID.
 *   The ray of sub-sample k of pixel (x, buffer row r), W x H the image:
 *     ky = H-1-r;   u = ((float)x + jx) / (float)(W-1);   v = ((float)ky + jy) / (float)(H-1);   rd = ((llc + h*u) + vert*v) - o
 *     -- make_camera_ray_jittered (:941-968) as the G-buffer pass forms it; on the CPU the oracle's camera-ray function (oracle/dsrt_oracle.h) with cam, x, ky, W, H, jx, jy.
 *   Its hit is scene_hit(ray, 0.001f, 1e9f); "sees the Sun" is DSRT_GB_SUN_VISIBLE's rule applied to that sub-sample's own hit.
 *   The representative: among the sub-samples that hit, the one with the smallest integer key, ties to the smaller k:
 *     GRID  key = (2i+1-S)^2 + (2j+1-S)^2          DIAGONAL  key = (2k+1-n)^2          (the squared distance from the pixel centre, in units of half a cell)
 *   CONSEQUENCE: for an odd S (an odd n) the centre sub-sample has key 0 and jx = jy = 0.5f exactly -- (float)((S-1)/2) + 0.5f is exactly S/2, and (S/2) / S is exactly
 *   0.5f -- so wherever the centre ray hits, `rep` is dsrt_render_gbuffer's pixel bit for bit, and samples = 1 (either pattern) IS the G-buffer.
 *
 * OUTPUTS.  DsrtCoverage holds DEVICE buffers of width*height elements in image order, each optional (NULL = not written):
 *   hits        u8        number of sub-samples that hit, 0..64
 *   alpha       f32       (float)hits / (float)n, one IEEE division
 *   mask        u64       bit k set iff sub-sample k hit
 *   sun_hits, sun_alpha, sun_mask    u8, f32, u64    the same for "hit and sees the Sun"; all 0 when the sun is disabled
 *   class_hits  u8 x classes->count per pixel (pixel-major)    sub-samples whose hit is a triangle with prim_id in class c:
 *                         prim >= first[c] && (uint32_t)(prim - first[c]) < (uint32_t)num[c] -- the range rule of TEMPORAL ACCUMULATION WITH BODIES; classes may
 *                         overlap or leave triangles out; spheres belong to no class.  dsrt_host_scene_body_range per body gives per-body masks.
 *   rep         a DsrtGBuffer: every G-buffer channel of the representative sub-sample (the table of GROUND-TRUTH G-BUFFER, with that sub-sample's ray);
 *               the miss values of that table when nothing hit.
 * The shadow rays are traced only when a sun output or rep.flags is asked for.
 *
 * dsrt_render_coverage: dsrt_render_gbuffer's envelope -- uses desc->width / height only; asynchronous on `stream` unless `stats` is given (then kernel_ms,
 *   waves_launched, device_flags); waits for the context's previous launch, the next launch waits for it; camera, sun, scene and working buffers are left as they were.
 *   DSRT_ERR_INVALID: what dsrt_render_gbuffer refuses; a NULL cov_desc or cov; no output at all; a pointer not aligned to its element (4 bytes for f32 and i32, 8 for
 *   u64); a pattern or `samples` outside the above; classes->count outside 0..16; a negative num; class_hits given without classes (or with count 0).
 *   DSRT_ERR_NO_SCENE before an upload.  A refused call touches no buffer.
 * dsrt_render_coverage_to_host: the same into HOST buffers, synchronously.
 * dsrt_coverage_defaults: DIAGONAL, 64 -- the pattern that COVERAGE DEMODULATION (DENOISER) wants.
 */
#define DSRT_COVERAGE_GRID     0
#define DSRT_COVERAGE_DIAGONAL 1
typedef struct DsrtCoverageDesc { int pattern; int samples; } DsrtCoverageDesc;
typedef struct DsrtCoverageClasses { int count /* 0..16 */; int first[16]; int num[16]; } DsrtCoverageClasses;
typedef struct DsrtCoverage {
    uint8_t*  hits;
    float*    alpha;
    uint64_t* mask;
    uint8_t*  sun_hits;
    float*    sun_alpha;
    uint64_t* sun_mask;
    uint8_t*  class_hits;
    DsrtGBuffer rep;
} DsrtCoverage;
void dsrt_coverage_defaults(DsrtCoverageDesc* out);
int dsrt_render_coverage(DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtCoverageDesc* cov_desc, const DsrtCoverageClasses* classes /* NULL ok */,
                         const DsrtCoverage* cov, void* stream, DsrtStats* stats);
int dsrt_render_coverage_to_host(DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtCoverageDesc* cov_desc, const DsrtCoverageClasses* classes,
                                 const DsrtCoverage* cov, DsrtStats* stats);

/*
 * RAY QUERIES.  Caller-supplied rays against the resident scene: for ray i, the reference's scene_hit(ray_i, t_min_i, t_max_i) (src/gpu_render.cu:509-551),
 * bit for bit -- the triangle walk on the REFERENCE tree (also when the certified second tree is resident), then the spheres in order; equal t is accepted,
 * so ties resolve by the reference's visit order.  t_min reaches every place the reference uses it (box entry, the triangle test, both sphere roots); t_max is
 * the initial closest distance.  Rays are in the MODEL frame (dsrt_pose_points_to_model / dsrt_pose_dirs_to_model take pose-file coordinates there).
 *
 * One lane per ray, in the order given: the walk is fastest when neighbouring rays are coherent (similar origins and directions), and ordering them is the
 * caller's business -- the library does not sort.
 *
 * Channels (DsrtRayHits, each optional, NULL = not written; `count` elements of the type and count of the G-buffer table above):
 *   t, range (t * sqrtf(dot(d, d))), position, normal, uv, albedo, prim_id (triangle index, -2 - s for sphere s), material_id, flags,
 *   on a miss +inf / +inf / 0 / 0 / 0 / 0 / -1 / -1 / 0.  flags: DSRT_GB_HIT, DSRT_GB_FRONT_FACE, DSRT_GB_SPHERE; DSRT_GB_SUN_VISIBLE is never set.
 *
 * Modes: DSRT_TRACE_CLOSEST, the closest hit and every channel asked for.  DSRT_TRACE_ANY, occlusion: `flags` only (any other channel is DSRT_ERR_INVALID),
 * DSRT_GB_HIT iff scene_hit would report a hit; the walk stops at the first accepted triangle.
 */
typedef struct DsrtRays {            /* DEVICE pointers for dsrt_trace_rays, HOST pointers for the _to_host form */
    const float* origins;            /* count x 3, model frame (the frame GPUScene lives in)             */
    const float* dirs;               /* count x 3, need not be normalised (t is in units of |dir|)       */
    const float* t_min;              /* count, or NULL = 0.001f                                          */
    const float* t_max;              /* count, or NULL = 1e9f                                            */
} DsrtRays;

typedef struct DsrtRayHits {         /* every channel optional (NULL = not written); per-ray values as the G-buffer table defines them */
    float*   t;
    float*   range;
    float*   position;
    float*   normal;
    float*   uv;
    float*   albedo;
    int32_t* prim_id;
    int32_t* material_id;
    uint8_t* flags;
} DsrtRayHits;

#define DSRT_TRACE_CLOSEST 0
#define DSRT_TRACE_ANY     1

/* Trace `count` rays from DEVICE buffers into DEVICE buffers.
 * DSRT_ERR_INVALID: a NULL ctx, rays, hits, origins or dirs; count < 0; an unknown mode; no output channel; a channel other than flags with DSRT_TRACE_ANY;
 * a pointer not 4-byte aligned; an output range that overlaps an input range.  DSRT_ERR_NO_SCENE before an upload.  count == 0: DSRT_OK, nothing launched.
 * Asynchronous on `stream` unless `stats` is given; then the call synchronises and fills kernel_ms, waves_launched and device_flags (the rest is 0), and
 * returns DSRT_ERR_DEVICE_FLAG when the kernel raised a status flag.  Like dsrt_render_gbuffer, the call waits for the context's previous launch, the next
 * launch waits for it, and the context's camera, sun and working buffers are left untouched. */
int dsrt_trace_rays(DsrtContext* ctx, int count, const DsrtRays* rays, int mode, const DsrtRayHits* hits, void* stream, DsrtStats* stats);
/* The same from HOST buffers into HOST buffers, synchronously. */
int dsrt_trace_rays_to_host(DsrtContext* ctx, int count, const DsrtRays* rays, int mode, const DsrtRayHits* hits, DsrtStats* stats);

/*
 * SAMPLE SETS (rng_mode 1; definitions with DsrtRenderDesc.rng_mode above): progressive preview, time-budgeted rendering, sample sharding between contexts,
 * streams or devices, and a per-pixel noise estimate.  The caller owns the sums; every accumulate launch ADDS to them.
 *   dsrt_render_accumulate: renders {first + j*stride : 0 <= j < count} of every pixel of the frame `desc` plans (desc->spp samples), with the context's camera
 *     and sun, into acc->sum (and acc->sum_sq when it is not NULL: the kernel that also sums squared samples is used only then).  Culled tiles get no additions.
 *     Asynchronous on `stream` unless `stats` is given (then as dsrt_render: synchronises and fills it; `samples` counts this launch's samples in a counting
 *     build).  collect_counters, checked, math_mode, tune and the certified second tree work as in dsrt_render.
 *     DSRT_ERR_INVALID: a NULL ctx, desc, acc or acc->sum; rng_mode != 1; shard_count > 1; first < 0, count < 1, stride < 1, first + (count-1)*stride >= spp.
 *     DSRT_ERR_NO_SCENE before an upload.  A refused call touches no buffer.
 *   dsrt_resolve_accumulated: the image of the sums after `samples_done` samples per pixel (rgb8, f32 as dsrt_render's; either may be NULL) and, if
 *     d_var_of_mean is not NULL, the variance of the mean (width*height*3 floats, needs acc->sum_sq and samples_done >= 2).  Waits for the context's last launch.
 *     DSRT_ERR_INVALID: a NULL ctx, desc, acc or acc->sum; rng_mode != 1; shard_count > 1; samples_done < 1; no output; the variance without sum_sq or with
 *     samples_done < 2.  Needs no scene.
 * The _to_host forms take HOST buffers (sums in and out, images out) and are synchronous.
 */
typedef struct DsrtAccum {          /* DEVICE buffers (HOST for the _to_host forms), width*height*3 uint64 each, image order (top row first), as dsrt_render's */
    uint64_t* sum;                  /* required: per-channel sums of q (units of 2^-20); the caller zeroes it once, every launch ADDS */
    uint64_t* sum_sq;               /* optional: per-channel sums of sq as defined above; NULL = the second moment is not summed */
} DsrtAccum;
int dsrt_render_accumulate(DsrtContext* ctx, const DsrtRenderDesc* desc, int first, int count, int stride, const DsrtAccum* acc, void* stream, DsrtStats* stats);
int dsrt_render_accumulate_to_host(DsrtContext* ctx, const DsrtRenderDesc* desc, int first, int count, int stride, const DsrtAccum* h_acc, DsrtStats* stats);
int dsrt_resolve_accumulated(DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtAccum* acc, int samples_done, uint8_t* d_rgb8, float* d_f32,
                             float* d_var_of_mean, void* stream);
int dsrt_resolve_accumulated_to_host(DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtAccum* h_acc, int samples_done, uint8_t* h_rgb8, float* h_f32,
                                     float* h_var_of_mean);

/*
 * ADAPTIVE SAMPLING (rng_mode 1, on top of SAMPLE SETS): stop sampling the pixels whose mean has converged and spend the launches on the others.  Three primitives
 * and a driver; every pixel's value stays defined by the set of its samples that were rendered, whichever launches rendered them.
 *   dsrt_render_accumulate_masked: dsrt_render_accumulate for a subset of the pixels.  d_mask: width*height bytes, image order (top row first), nonzero = active.
 *     For every active pixel the launch adds exactly what dsrt_render_accumulate(first, count, stride) adds to acc->sum (and acc->sum_sq when given); for every
 *     other pixel it adds nothing and writes nothing.  d_n (optional): width*height uint32, image order, the pixels' sample counts: `count` is added to d_n[p] of
 *     every active pixel -- pixels of culled tiles included: their samples are black, their sums get no addition, and the count does not depend on culling.
 *     An all-zero mask is a valid launch that changes nothing.  The mask is read on the device, in stream order.
 *     DSRT_ERR_INVALID: everything dsrt_render_accumulate refuses; a NULL mask; collect_counters != 0 (masked launches use the production and checked kernels only).
 *     DSRT_ERR_NO_SCENE before an upload.  A refused call touches no buffer.
 *   dsrt_select_unconverged: the mask of the pixels that still need samples.  Per pixel with n = d_n[p], per channel with the sums S = acc->sum, S2 = acc->sum_sq,
 *     in double, in exactly this order, every operation correctly rounded (no fused operations, no sqrt):
 *         s = (double)S * 2^-20;  s2 = (double)S2 * 2^-20;  v = (s2 - s*s/n) / (n - 1);  v = v > 0 ? v : 0;  vm = v / n;  m = s / n;
 *         r = m > (double)floor ? m : (double)floor;  lim = (double)rel_tol * r;  ok = vm <= lim*lim
 *     i.e. the standard error of the mean is at most rel_tol times the mean (or times `floor`, for dark pixels).  A pixel with n < 2 is never converged;
 *     converged = ok_r && ok_g && ok_b;  mask[p] = n < n_max && (n < n_min || !converged) ? 1 : 0.  h_active (optional, HOST): the number of bytes set; the call
 *     synchronises `stream` when it is given.  Waits for the context's last launch.  Needs no scene.
 *     DSRT_ERR_INVALID: a NULL ctx, desc, acc, acc->sum, acc->sum_sq, d_n or d_mask; rng_mode != 1; shard_count > 1; rel_tol or floor negative or NaN.
 *     Stopping on a pixel's own estimate is slightly biased, as with every adaptive sampler: a pixel whose first n_min samples are all alike has v = 0 and stops
 *     at n_min although later samples might have differed (an edge the first samples missed).  n_min is the guard against that: choose it with the scene in mind.
 *   dsrt_resolve_accumulated_counts: dsrt_resolve_accumulated's arithmetic with the pixel's own n = d_n[p] in place of samples_done.  A pixel with n == 0 resolves
 *     to zero bytes, +0.0f and variance +0.0f; a pixel with n == 1 has variance +0.0f.  Refusals as dsrt_resolve_accumulated's (the variance needs acc->sum_sq), and a NULL d_n.
 *   dsrt_render_adaptive: the frame `desc` plans (desc->spp samples) in up to P = passes passes, 1 <= P <= min(spp, 64).  Pass p is the interleaved set
 *     (first p, count len(range(p, spp, P)), stride P), which keeps every pixel's samples spread over its area.  Passes < min_passes (1 <= min_passes <= P) cover every
 *     pixel; from pass min_passes - 1 on, each pass but the last is followed by dsrt_select_unconverged(rel_tol, floor, n_min 0, n_max UINT32_MAX) -- one 4-byte
 *     readback -- and the next pass is a masked launch over that mask.  The loop ends when no pixel is active or the passes run out; then
 *     dsrt_resolve_accumulated_counts writes the outputs (at least one of d_rgb8, d_f32, d_var_of_mean).  acc (with sum_sq) and d_n are the caller's, zeroed by the
 *     caller: afterwards they hold the frame's sums and every pixel's sample count.  stats (optional): passes_run, active[p] = pixels pass p rendered,
 *     samples_total = the sum over the passes of active[p] * count_p.  Synchronises `stream` after every test.  With desc->checked the status word of every pass
 *     is read behind it (one more synchronisation per pass) and the first pass that raised it ends the call with DSRT_ERR_DEVICE_FLAG, as the primitives with
 *     `stats` do; sums and counts then hold the passes up to and including that one, and no output is written.
 *     DSRT_ERR_INVALID: what the three calls refuse; passes < 1, > spp or > 64; min_passes < 1 or > passes.
 * The _to_host forms take HOST buffers and are synchronous; dsrt_render_adaptive_to_host keeps the sums on the device and returns the counts in h_n (optional).
 */
typedef struct DsrtAdaptive { int passes; int min_passes; float rel_tol; float floor; } DsrtAdaptive;
typedef struct DsrtAdaptiveStats { int passes_run; uint64_t samples_total; uint32_t active[64]; } DsrtAdaptiveStats;
int dsrt_render_accumulate_masked(DsrtContext* ctx, const DsrtRenderDesc* desc, int first, int count, int stride, const DsrtAccum* acc, const uint8_t* d_mask,
                                  uint32_t* d_n, void* stream, DsrtStats* stats);
int dsrt_render_accumulate_masked_to_host(DsrtContext* ctx, const DsrtRenderDesc* desc, int first, int count, int stride, const DsrtAccum* h_acc, const uint8_t* h_mask,
                                          uint32_t* h_n, DsrtStats* stats);
int dsrt_select_unconverged(DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtAccum* acc, const uint32_t* d_n, float rel_tol, float floor, uint32_t n_min,
                            uint32_t n_max, uint8_t* d_mask, uint32_t* h_active, void* stream);
int dsrt_resolve_accumulated_counts(DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtAccum* acc, const uint32_t* d_n, uint8_t* d_rgb8, float* d_f32,
                                    float* d_var_of_mean, void* stream);
int dsrt_render_adaptive(DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtAdaptive* adaptive, const DsrtAccum* acc, uint32_t* d_n, uint8_t* d_rgb8, float* d_f32,
                         float* d_var_of_mean, void* stream, DsrtAdaptiveStats* stats);
int dsrt_render_adaptive_to_host(DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtAdaptive* adaptive, uint32_t* h_n, uint8_t* h_rgb8, float* h_f32,
                                 float* h_var_of_mean, DsrtAdaptiveStats* stats);

/*
 * DENOISER (rng_mode 1, on top of SAMPLE SETS and the G-BUFFER): an edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) in the variance-guided form of SVGF,
 * on a single frame.  It reconstructs an image from the samples already taken: the per-pixel mean and its variance come from the sums, the edge-stopping guides
 * (normal, position, albedo, range of the pixel-centre ray) from dsrt_render_gbuffer.  What it computes is written out here in full; it uses correctly rounded
 * fp32 operations only, so a CPU reproduces every bit (tests/_denoise_model.py).
 *
 * THE ARITHMETIC.  fp32 unless marked double; every operation one correctly rounded IEEE operation, never contracted, in the order written; sqrtf and / are the IEEE
 * ones; the constants are float literals.
 *     L(x) = (0.2126f*x.r + 0.7152f*x.g) + 0.0722f*x.b            dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z
 *     h = {1/16, 1/4, 3/8, 1/4, 1/16}  (the B3 spline)            k3 = {1/4, 1/2, 1/4}
 *   Start, per pixel p with n its sample count (samples_done, or d_n[p]):
 *     c   = dsrt_resolve_accumulated_counts' mean: (float)((double)sum * (1.0 / 2^20 / n)), in double, converted once; +0 for n = 0
 *     v   = its variance of the mean, as defined with DsrtRenderDesc.rng_mode; +0 for n < 2
 *     F_p = (range_p <= FLT_MAX) && n >= 2: "filterable" (a NaN range is not)
 *   Iteration i = 0 .. iterations-1, step s = 1 << i, takes (c, v) to (c', v'), reading the previous iteration's images only:
 *     !F_p:  c' = c, v' = v, bit for bit.  Otherwise
 *     g     = sum over ey = -1..1 (outer, ascending), ex = -1..1 of (k3[ex+1]*k3[ey+1]) * L(v_q), q = p + (ex, ey) CLAMPED to the image, starting from +0;
 *             every pixel counts, filterable or not
 *     den_l = sigma_l * sqrtf(g) + 0x1p-20f;   den_z = sigma_z * range_p;   lp = L(c_p)
 *     taps dy = -2..2 (outer), dx = -2..2, q = p + s*(dx, dy) in buffer coordinates (row 0 the top row); a tap outside the image or with !F_q is skipped; else
 *         wn = fmaxf(dot(N_p, N_q), 0.0f);  normal_power_log2 times: wn = wn * wn;
 *         D  = X_q - X_p;   ez = fabsf(dot(N_p, D)) / den_z;
 *         el = fabsf(L(c_q) - lp) / den_l;
 *         da = A_q - A_p;   ea2 = dot(da, da) / (sigma_a * sigma_a);
 *         w  = ((h[dx+2]*h[dy+2]) * wn) / (((1.0f + ez*ez) * (1.0f + el*el)) * (1.0f + ea2));
 *         sw += w;   sc.k += w * c_q.k;   sv.k += (w*w) * v_q.k;                    (k = r, g, b; all sums start at +0.0f)
 *     sw > 0:  c'.k = sc.k / sw,  v'.k = sv.k / (sw*sw);  otherwise p is copied through
 *   Output, after the last iteration: d_linear = c, d_var = v; d_rgb8 and d_f32 are dsrt_resolve_accumulated's tone map and 8-bit store applied to c
 *   (desc->math_mode chooses powf as it does there).
 * The Cauchy weights 1/(1+e^2) stand where SVGF has exp(-e): expf is in no correctly rounded set, and the filter does not need it.  The geometry term is the distance
 * of q's hit point from p's tangent plane relative to p's range: zero along a flat oblique surface, which a depth difference gets wrong.
 * BACKGROUND AND SILHOUETTE: a pixel whose centre ray misses is never touched and never contributes -- space stays black and the silhouette stays where the renderer
 * put it; so the partially covered pixels just OUTSIDE the silhouette (centre ray misses, some samples hit) stay unfiltered
 * -- unless the call is given their coverage: COVERAGE DEMODULATION below.
 * Guides must be finite wherever `range` is finite; the call does not check.
 *
 * dsrt_denoise_accumulated: at least one of d_rgb8 (bytes), d_f32, d_linear, d_var (floats), each width*height*3 elements.  Asynchronous on `stream`; like
 *   dsrt_resolve_accumulated and dsrt_render_gbuffer it waits for the context's previous launch, the next launch waits for it, it needs no scene, and the context's
 *   camera, sun and render buffers are left as they were.  Sums, counts and guides are read only.  Working memory (112 bytes per pixel: the packed guides and two
 *   colour / variance pairs to ping-pong) belongs to the context: allocated on first use, grown for a larger frame, freed by dsrt_ctx_destroy.
 *   DSRT_ERR_INVALID: a NULL ctx, desc, acc, acc->sum, acc->sum_sq, guides, guide channel or params; rng_mode != 1; shard_count > 1; width or height < 2;
 *   samples_done < 2 when d_n is NULL; iterations outside [0, 6]; normal_power_log2 outside [0, 8]; a sigma that is not > 0 (NaN is refused); no output; a pointer not
 *   aligned to its element; an output range that overlaps an input range or another output.  A refused call touches no buffer.
 * dsrt_denoise_accumulated_to_host: the same from HOST buffers into HOST buffers, synchronously.
 * dsrt_render_denoised_to_host: the convenience form -- desc->spp samples with second moments, the G-buffer of the current camera, and the call above.
 *   DSRT_ERR_NO_SCENE before an upload.  stats (optional): the accumulate launch's, as dsrt_render_accumulate fills them; spp must be at least 2.
 * dsrt_denoise_defaults: iterations 5, normal_power_log2 5, sigma_l 1, sigma_z 0.01, sigma_a 0.1.  sigma_l was first set to SVGF's 4; on the parity scenes at 8 and
 *   16 samples per pixel that blurs the station's sun shadows until the error RISES with the iterations (1.2 times the unfiltered error after five), while with 1 --
 *   a tap's weight halves at one standard deviation of luminance -- it falls to about half and stays there (tests/test_denoise_host.py).
 *
 * COVERAGE DEMODULATION (dsrt_denoise_accumulated_coverage).  Space is exactly black, so a pixel's mean is alpha x (the radiance of its covered part), alpha the
 * share of its samples that hit.  With a per-pixel alpha (d_alpha, one float per pixel: the `alpha` of a DIAGONAL coverage pass, the renderer's own measure) the
 * filter works on the covered part and the result is multiplied by alpha again; with the `rep` channels of that pass as guides, a pixel whose centre ray misses but
 * whose samples hit becomes filterable.  With a = alpha_p:
 *     F_p = (range_p <= FLT_MAX) && n >= 2 && a >= alpha_min          (a NaN alpha is not filterable)
 *   Start, for F_p:    c.k = c.k / a;   aa = a * a;   v.k = v.k / aa.   A pixel that is not F_p keeps c and v bit for bit, and is never a tap.
 *   Iterations: the ones above, untouched.
 *   Output, for F_p:   c.k = c'.k * a;   v.k = v'.k * aa   (aa = a * a again);  d_linear and d_var are these, and the tone map is applied to that c.
 * alpha_min must be in (0, 1] (a NaN is refused); d_alpha is 4-byte aligned and overlaps no output.  Everything else is dsrt_denoise_accumulated's.  Two identities:
 * d_alpha == NULL is dsrt_denoise_accumulated bit for bit (alpha_min is then not looked at beyond its check), and so is an alpha that is 1.0f everywhere with any
 * legal alpha_min, since x / 1 and x * 1 are exact.
 * dsrt_render_denoised_coverage_to_host: the convenience form -- desc->spp samples with second moments, a DIAGONAL coverage pass (cov_desc NULL = dsrt_coverage_defaults;
 *   a GRID pattern is refused) whose alpha and rep channels are the alpha and the guides, and the call above.  h_alpha (optional) receives that alpha.
 * dsrt_denoise_coverage_alpha_min: the default alpha_min (DESIGN.md section 4 says how it was chosen).
 */
typedef struct DsrtDenoiseGuides {   /* DEVICE (HOST for _to_host) buffers, width*height elements, image order: channels of DsrtGBuffer */
    const float* normal;             /* x3 */
    const float* position;           /* x3 */
    const float* albedo;             /* x3 */
    const float* range;              /* x1, +inf on a miss */
} DsrtDenoiseGuides;
typedef struct DsrtDenoise { int iterations; int normal_power_log2; float sigma_l, sigma_z, sigma_a; } DsrtDenoise;
void dsrt_denoise_defaults(DsrtDenoise* out);
int  dsrt_denoise_accumulated(DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtAccum* acc, int samples_done, const uint32_t* d_n /* NULL = samples_done for every pixel */,
                              const DsrtDenoiseGuides* guides, const DsrtDenoise* params, uint8_t* d_rgb8, float* d_f32, float* d_linear, float* d_var, void* stream);
int  dsrt_denoise_accumulated_to_host(DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtAccum* h_acc, int samples_done, const uint32_t* h_n,
                                      const DsrtDenoiseGuides* h_guides, const DsrtDenoise* params, uint8_t* h_rgb8, float* h_f32, float* h_linear, float* h_var);
int  dsrt_render_denoised_to_host(DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtDenoise* params, uint8_t* h_rgb8, float* h_f32, float* h_linear, float* h_var,
                                  DsrtStats* stats);
float dsrt_denoise_coverage_alpha_min(void);
int  dsrt_denoise_accumulated_coverage(DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtAccum* acc, int samples_done, const uint32_t* d_n, const DsrtDenoiseGuides* guides,
                                       const float* d_alpha /* NULL = dsrt_denoise_accumulated */, float alpha_min, const DsrtDenoise* params, uint8_t* d_rgb8, float* d_f32,
                                       float* d_linear, float* d_var, void* stream);
int  dsrt_denoise_accumulated_coverage_to_host(DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtAccum* h_acc, int samples_done, const uint32_t* h_n,
                                               const DsrtDenoiseGuides* h_guides, const float* h_alpha, float alpha_min, const DsrtDenoise* params, uint8_t* h_rgb8,
                                               float* h_f32, float* h_linear, float* h_var);
int  dsrt_render_denoised_coverage_to_host(DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtCoverageDesc* cov_desc, float alpha_min, const DsrtDenoise* params,
                                           uint8_t* h_rgb8, float* h_f32, float* h_linear, float* h_var, float* h_alpha, DsrtStats* stats);

/*
 * TEMPORAL ACCUMULATION (rng_mode 1, on top of the DENOISER): the other half of SVGF -- a frame's mean and variance blended with the history of the frames before it,
 * reprojected through the previous camera, before the a-trous iterations run.  The scene is static in the model frame, so a pixel's G-buffer position IS the
 * motion vector's source; the variance of the mean comes from the sample sums, so no temporal moment estimate is needed.  One light kernel per frame multiplies the
 * effective sample count of every surface point that stays visible.  As a by-product the stage yields the ground-truth correspondence between two frames
 * (d_prev_xy: optical-flow ground truth).  Like the denoiser it uses correctly rounded fp32 operations only: tests/_temporal_model.py reproduces every bit.
 *
 * THE ARITHMETIC.  All fp32; every operation one correctly rounded IEEE operation, never contracted, in the order written; dot and L are the DENOISER's.
 *   History: one caller-owned DEVICE buffer per frame, width*height records of 16 floats (64 bytes) in image order (top row first), 16-byte aligned:
 *       {c.r, c.g, c.b, m,   v.r, v.g, v.b, 0,   N.x, N.y, N.z, 0,   X.x, X.y, X.z, 0}
 *     c the accumulated linear mean, v its variance, m its weight in samples (m = +0: a record that must never be used), N and X the G-buffer normal and position
 *     of the frame that wrote the record.  The caller ping-pongs two buffers; `next` must not overlap `prev` or any input.
 *   Start, per pixel p = (x, y) (y the buffer row, 0 the top row): the DENOISER's Start values c, v, n, F_p and the current frame's guides N_p, X_p, range_p.
 *     The projection runs when a previous frame is given and range_p <= FLT_MAX; C is the previous frame's GPUCamera, W = width, H = height:
 *       D  = X_p - C.origin;  e = C.lower_left_corner - C.origin                                          (componentwise)
 *       a  = dot(D, C.u);  b = dot(D, C.v);  cc = dot(D, C.w)
 *       eu = dot(e, C.u);  ev = dot(e, C.v);  ew = dot(e, C.w);  hu = dot(C.horizontal, C.u);  vv = dot(C.vertical, C.v)
 *       k  = ew / cc;                                       !(k > 0): not projected                        (behind the camera, or NaN)
 *       s  = (a*k - eu) / hu;   t = (b*k - ev) / vv
 *       fx = s*(float)(W-1) - 0.5f;   fy = (float)(H-1) - (t*(float)(H-1) - 0.5f)
 *       !(fx > -1.0f && fx < (float)W && fy > -1.0f && fy < (float)H): not projected
 *     -- the inverse of the G-buffer's pixel-centre ray (u = (x + 0.5) / (W - 1)), in buffer coordinates.  A pixel has NO HISTORY when no previous frame is given,
 *     when !F_p, when it is not projected, or when the taps below do not find enough support.  For a projected pixel with F_p:
 *       x0 = floorf(fx);  y0 = floorf(fy);  wx = fx - x0;  wy = fy - y0;  ox = 1.0f - wx;  oy = 1.0f - wy
 *     Taps q, in the order (x0, y0), (x0+1, y0), (x0, y0+1), (x0+1, y0+1), with the weights bq = ox*oy, wx*oy, ox*wy, wx*wy.  A tap is skipped when it lies outside
 *     the image, or !(m_q > 0), or !(dot(N_p, N_q) >= normal_cos_min), or !(fabsf(dot(N_p, X_q - X_p)) <= plane_tol * range_p); otherwise (sums from +0.0f)
 *       sw += bq;   sc.k += bq*c_q.k;   sv.k += bq*v_q.k;   sm += bq*m_q                                    (k = r, g, b)
 *     !(sw >= min_support): no history.
 *     Occluder guard, for the same pixels: over the block qx = x0-1 .. x0+2, qy = y0-1 .. y0+2 (the part of it inside the image), a record with m_q > 0 and
 *       dot(N_p, X_q - X_p) > plane_tol * range_p
 *     -- a surface the previous frame saw IN FRONT of this pixel's tangent plane, within two pixels of where its point projects -- means no history, unless one
 *     of the accumulated taps has bq >= 0.99f: that tap's centre ray all but coincides with the ray to X_p (within a hundredth of a pixel) and it saw the pixel's
 *     surface, which proves the point visible (a camera that has not moved: every pixel).  The guard is what catches an occluder thinner than a pixel that passed
 *     between the four taps' centre rays (see dsrt_temporal_defaults below).
 *   Blend, with history:
 *       ch = sc/sw;  vh = sv/sw;  mh = sm/sw;  nf = (float)n
 *       alpha = fmaxf(nf / (nf + mh), alpha_min);   beta = 1.0f - alpha
 *       c'.k = beta*ch.k + alpha*c.k;   v'.k = (beta*beta)*vh.k + (alpha*alpha)*v.k;   m' = nf / alpha
 *     without: c' = c and v' = v bit for bit, m' = F_p ? nf : +0.
 *   Outputs of the stage: next[p] = {c', m', v', 0, N_p, 0, X_p, 0}; the DENOISER's iterations then run on (c', v') with the unchanged F_p, and its outputs (rgb8, f32,
 *     linear, var) are as there.  d_prev_xy (optional, 2 floats per pixel) receives (fx, fy) for every projected pixel -- whether the taps found history does not
 *     matter -- and two quiet NaNs (0x7FC00000) otherwise: the position of the pixel's surface point in the previous frame, occluded there or not.  d_weight
 *     (optional, 1 float per pixel) receives m'.
 * WHAT THE BLEND ASSUMES.  The variance blend treats the frames' estimates as independent: that holds only when the frames were rendered with DIFFERENT SEEDS (with
 * one seed, sample k of pixel p draws the same Philox sub-sequence in every frame and the frames' noise is correlated: the variance then understates the error).
 * The history is radiance seen from the previous viewpoints under the previous Sun: view-dependent shading (metal, glass) and a moving Sun make it lag behind the
 * current frame.  alpha_min is the guard against that lag: the current frame never weighs less than alpha_min, so the history fades with about 1/alpha_min frames.
 *
 * dsrt_denoise_temporal: dsrt_denoise_accumulated with the stage above between its Start and its first iteration.  prev_camera (HOST) and d_history_prev are both
 *   NULL (the first frame of a sequence: every pixel is without history) or both given; d_history_next is required.  Stream order, waiting, working memory and "needs
 *   no scene" as dsrt_denoise_accumulated.  DSRT_ERR_INVALID: what dsrt_denoise_accumulated refuses; only one of prev_camera / d_history_prev; a NULL d_history_next
 *   or DsrtTemporal; alpha_min outside [0, 1]; normal_cos_min outside [-1, 1]; plane_tol or min_support not > 0; min_support > 1; a NaN parameter; a history buffer
 *   not 16-byte aligned (d_prev_xy, d_weight: 4-byte); d_history_next, d_prev_xy or d_weight overlapping d_history_prev, an input, an output or each other.  A refused call touches no buffer.
 * dsrt_denoise_temporal_to_host: the same from HOST buffers into HOST buffers (the histories too), synchronously.
 * dsrt_render_denoised_temporal_to_host: the convenience form -- dsrt_render_denoised_to_host's three steps with the temporal stage, the two history buffers and the
 *   previous camera kept by the CONTEXT (allocated on first use, freed by dsrt_ctx_destroy; a clone has its own).  The context starts a new sequence (no history)
 *   when reset != 0, when width or height differ from the previous call's, and after a scene upload; otherwise what it computes is exactly the explicit chain of
 *   dsrt_denoise_temporal calls.  The caller changes desc->seed from frame to frame (see above).  A failed call leaves the sequence where it was.
 * dsrt_temporal_defaults: alpha_min 0.1 (ten frames of memory), normal_cos_min 0.9 (about 26 degrees), plane_tol 0.01 (the denoiser's sigma_z), min_support 0.9.
 *   min_support was first set to 0.25 -- one full tap out of four.  On the station at 200 x 112 that is harmful: a pixel on a silhouette or behind a thin truss then
 *   takes its whole history from the one or two taps that lie on its surface, whose means hold other fractions of background than its own, and over the pixels with
 *   history the error after the a-trous iterations is 1.5 times the single-frame denoiser's.  With 0.9 -- the footprint must lie on the pixel's surface almost
 *   entirely -- it is 0.76 times (0.44 times on the textured room), and three quarters of the visible surface points still find history.  The other three values
 *   are the reasoned ones: the measurements do not depend on them within wide bounds.
 *   THE OCCLUDER GUARD was added on the same evidence.  Of the station's points that the previous camera could not see, 12 % still found history with the four tap
 *   tests alone, whatever their parameters (49 % with min_support 0.25): the occluder there is a truss or an edge-on panel thinner than a pixel that passed between
 *   the four taps' centre rays, so that all four records show the pixel's own surface.  The previous G-buffer does see that occluder one or two pixels further
 *   along; with the guard 2 % find history (1 pixel of 41), 68 % of the visible points do (95 % in the textured room), and the error figures become 0.81 and 0.44.
 *   Its tolerance is plane_tol: what counts as off the plane for a tap counts as in front of it for the guard (tests/test_temporal_host.py).
 */
typedef struct DsrtTemporal { float alpha_min, normal_cos_min, plane_tol, min_support; } DsrtTemporal;
void dsrt_temporal_defaults(DsrtTemporal* out);
int  dsrt_denoise_temporal(DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtAccum* acc, int samples_done, const uint32_t* d_n, const DsrtDenoiseGuides* guides,
                           const GPUCamera* prev_camera /* HOST */, const float* d_history_prev, float* d_history_next, const DsrtTemporal* temporal, const DsrtDenoise* params,
                           uint8_t* d_rgb8, float* d_f32, float* d_linear, float* d_var, float* d_prev_xy, float* d_weight, void* stream);
int  dsrt_denoise_temporal_to_host(DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtAccum* h_acc, int samples_done, const uint32_t* h_n, const DsrtDenoiseGuides* h_guides,
                                   const GPUCamera* prev_camera, const float* h_history_prev, float* h_history_next, const DsrtTemporal* temporal, const DsrtDenoise* params,
                                   uint8_t* h_rgb8, float* h_f32, float* h_linear, float* h_var, float* h_prev_xy, float* h_weight);
int  dsrt_render_denoised_temporal_to_host(DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtDenoise* params, const DsrtTemporal* temporal, int reset, uint8_t* h_rgb8,
                                           float* h_f32, float* h_linear, float* h_var, float* h_prev_xy, DsrtStats* stats);

/*
 * TEMPORAL ACCUMULATION WITH BODIES (on top of TEMPORAL ACCUMULATION and MOVABLE RIGID BODIES): the stage above assumes a scene that is static in the model frame,
 * and a sequence with movable bodies is the one that most needs accumulated samples and flow ground truth.  The G-buffer gives every pixel's triangle, the host scene
 * every body's triangle range, and the caller owns the poses of both frames: the MOTION STAGE takes a pixel's surface point and normal back to where that material
 * point was in the previous frame, and the stage above -- projection, tap tests, occluder guard -- works on that.  tests/_motion_model.py reproduces every bit.
 *
 * THE ARITHMETIC.  All fp32; every operation one correctly rounded IEEE operation, never contracted, in the order written.
 *   Motion description (DsrtBodyMotion): bodies in 1 .. DSRT_MAX_BODIES; HOST arrays first_tri[bodies], num_tris[bodies] (as dsrt_host_scene_body_range gives them),
 *     poses_prev[12*bodies], poses_cur[12*bodies] (row-major 3 x 4, applied to the rest pose, as everywhere; entry 0 is ignored: body 0 never moves); prim_id, the
 *     G-buffer's int32 channel of the CURRENT frame (a DEVICE pointer; a HOST pointer in the _to_host form and in dsrt_body_motion_host).  poses_prev are the poses
 *     the scene had when history_prev was written.
 *   Body of a pixel: b(p) = the b >= 1 with first_tri[b] <= prim_id[p] < first_tri[b] + num_tris[b], otherwise 0 -- body 0's triangles, spheres (<= -2), misses (-1)
 *     and any other value.
 *   Moved: body b >= 1 is MOVED when any of its 12 pose floats differs (!=) between prev and cur.
 *   A pixel whose body is 0 or not moved: N' = N_p and X' = X_p bit for bit.
 *   A pixel on a moved body, c = the cur pose (c00 .. c22, translation ct), q = the prev pose (q00 .. q22, qt); the current rotation's transpose stands in for its
 *     inverse (an orthonormal R stays the caller's business, as in MOVABLE RIGID BODIES):
 *       d   = X_p - ct                                                                                   (componentwise)
 *       r.x = (c00*d.x + c10*d.y) + c20*d.z;   r.y with c01, c11, c21;   r.z with c02, c12, c22
 *       X'.x = ((q00*r.x + q01*r.y) + q02*r.z) + qt.x;   rows 1 and 2 likewise                            (the "point" rule of MOVABLE RIGID BODIES)
 *       m   = the same transpose product applied to N_p;   N' = the "normal" rule applied to m            (no translation, NOT renormalised)
 *   The stage: TEMPORAL ACCUMULATION with (N', X') in place of (N_p, X_p) wherever the pixel meets the previous frame -- D = X' - C.origin in the projection, both
 *     tap tests, the occluder guard.  The rest is as there: range_p, F_p, c, v and n are the current frame's, the tolerance stays plane_tol * range_p, and the `next`
 *     record stores the current N_p, X_p.
 *   Outputs: d_prev_xy is (fx, fy) of X' -- flow ground truth that includes the bodies' motion.  d_prev_position (optional, 3 floats per pixel) receives X' for every
 *     pixel with range_p <= FLT_MAX, whether or not a previous frame is given, and +0 otherwise.
 * With all poses equal the stage is the static one, bit for bit.  A body that enters or leaves the view, or that uncovers the station behind it, needs nothing of its
 * own: the record at the projected place shows another surface, and the tap tests and the guard reject it.
 * WHAT IS NOT FOLLOWED: SHADING.  A moving body's shadow moves across static pixels, and a body's own radiance changes as it turns to the Sun: the history lags there,
 * and alpha_min is the only guard of THIS stage.  TEMPORAL ACCUMULATION THAT FOLLOWS SHADING below carries the G-buffer's sun-visibility bit in the spare word of
 * the history record and rejects taps across a changed bit.
 *
 * dsrt_body_motion_host: the CPU statement of the motion rule over n points, no GPU involved: prim_id (HOST, n entries), normal and position (3 floats per point)
 *   give prev_normal = N' and prev_position = X' (either may be NULL; they may not overlap the inputs).  DSRT_ERR_INVALID: what is refused of a DsrtBodyMotion below,
 *   n < 0, a NULL input, a pointer not 4-byte aligned.
 * dsrt_denoise_temporal_bodies: dsrt_denoise_temporal with the motion stage: `motion` after `guides`, d_prev_position after d_weight.  Stream order, waiting, working
 *   memory and "needs no scene" are unchanged; the motion's HOST arrays are read before the call returns.  DSRT_ERR_INVALID: what dsrt_denoise_temporal refuses; a
 *   NULL motion or a NULL member of it; bodies outside 1 .. 16; a negative first_tri or num_tris (first_tri + num_tris may be anything up to 2^32 - 2: the range
 *   test is the rule above for every int32 prim_id, on the host and on the device); ranges of bodies >= 1 that overlap; a pose entry of a body >= 1
 *   that is not finite; prim_id not 4-byte aligned, or overlapping an output; d_prev_position misaligned, or overlapping anything.  `motion` is validated on the first
 *   frame (prev NULL) too.  A refused call touches no buffer.
 * dsrt_denoise_temporal_bodies_to_host: the same from HOST buffers into HOST buffers, synchronously.
 * dsrt_ctx_set_temporal_bodies / dsrt_ctx_temporal_bodies: the switch of the convenience form, per context (a clone has its own, off), OFF by default; off
 *   is the behaviour described above: a pose update voids the context's sequence.  ON, and the resident scene has bodies: dsrt_scene_set_body_poses does not void the
 *   sequence, and dsrt_render_denoised_temporal_to_host asks its G-buffer for prim_id as well, runs the stage above with cur = the resident scene's current poses
 *   (a host copy kept with the shared scene; identity after dsrt_scene_upload_bodies) and prev = the poses of this context's last temporal frame, and records cur
 *   afterwards.  reset, a size change and an upload still start afresh.  The result is exactly the explicit chain of dsrt_denoise_temporal_bodies calls.
 */
typedef struct DsrtBodyMotion {
    int bodies;
    const int* first_tri;       /* HOST, [bodies] */
    const int* num_tris;        /* HOST, [bodies] */
    const float* poses_prev;    /* HOST, [12*bodies] */
    const float* poses_cur;     /* HOST, [12*bodies] */
    const int32_t* prim_id;     /* DEVICE (HOST in the host forms), one per pixel */
} DsrtBodyMotion;
int  dsrt_body_motion_host(const DsrtBodyMotion* motion, int n, const float* normal, const float* position, float* prev_normal, float* prev_position);
int  dsrt_denoise_temporal_bodies(DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtAccum* acc, int samples_done, const uint32_t* d_n, const DsrtDenoiseGuides* guides,
                                  const DsrtBodyMotion* motion, const GPUCamera* prev_camera /* HOST */, const float* d_history_prev, float* d_history_next,
                                  const DsrtTemporal* temporal, const DsrtDenoise* params, uint8_t* d_rgb8, float* d_f32, float* d_linear, float* d_var, float* d_prev_xy,
                                  float* d_weight, float* d_prev_position, void* stream);
int  dsrt_denoise_temporal_bodies_to_host(DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtAccum* h_acc, int samples_done, const uint32_t* h_n,
                                          const DsrtDenoiseGuides* h_guides, const DsrtBodyMotion* motion, const GPUCamera* prev_camera, const float* h_history_prev,
                                          float* h_history_next, const DsrtTemporal* temporal, const DsrtDenoise* params, uint8_t* h_rgb8, float* h_f32, float* h_linear,
                                          float* h_var, float* h_prev_xy, float* h_weight, float* h_prev_position);
int  dsrt_ctx_set_temporal_bodies(DsrtContext* ctx, int on);
int  dsrt_ctx_temporal_bodies(const DsrtContext* ctx);

/*
 * TEMPORAL ACCUMULATION THAT FOLLOWS SHADING (on top of TEMPORAL ACCUMULATION WITH BODIES and the G-BUFFER): the two stages above follow geometry.  When a body's
 * shadow crosses the station, or a body turns through its terminator, the history of a surface point holds radiance under the other sun state, and blending it in
 * is worse than the frame's own samples.  This stage keeps every record's SUN STATE -- the G-buffer's sun-visibility bit of the frame that wrote it -- in the spare
 * word after X, rejects taps of the other state, and (edge_guard) voids the history next to a shadow edge of either frame: a pixel that straddles the edge keeps its
 * pixel-centre bit while the edge moves by a fraction of a pixel.  tests/_shading_model.py reproduces every bit.
 *
 * THE ARITHMETIC.  All fp32; every operation one correctly rounded IEEE operation, never contracted, in the order written.  The stage is TEMPORAL ACCUMULATION WITH
 * BODIES with the additions below; a NULL `motion` means every pixel is body 0 (N' = N_p, X' = X_p): the static stage.
 *   Input: flags, the G-buffer's u8 channel of the CURRENT frame (DSRT_GB_HIT = 1, DSRT_GB_SUN_VISIBLE = 8), one byte per pixel.
 *   Sun state of a pixel:  s_p = range_p <= FLT_MAX ? ((flags_p & 8) ? 2.0f : 1.0f) : +0.0f              (2 lit, 1 in shadow, 0 unknown)
 *   Record: next[p] = {c', m', v', 0, N_p, 0, X_p, s_p}: word 15 holds the state, words 7 and 11 stay +0.  A record whose word 15 is 0 (-0 too) is UNKNOWN and matches
 *     every state: a record written by dsrt_denoise_temporal or dsrt_denoise_temporal_bodies is one, so a sequence may switch this stage on between two frames.
 *   State mismatch of a record q:  mis(q) = !(s_q == 0.0f || s_q == s_p)                                    (a NaN in the word mismatches; so does any stray value)
 *   Taps: after the plane test a tap is also skipped when mis(q).  Two more sums run over the taps that pass the three tests above it, whatever their state:
 *       swg += bq;   seen_g |= bq >= 0.99f
 *     found_geometry = swg >= min_support && (seen_g || !guarded): the decision of the stage above.  sw and seen count the taps that pass all four tests.
 *   Previous-frame edge, over the occluder guard's 4 x 4 block (the part of it inside the image):  edge_prev = any record with m_q > 0 and mis(q).
 *   Current-frame edge, over the 3 x 3 block around p (the part of it inside the image):  edge_cur = any r with (flags_r & 1) and (flags_r & 8) != (flags_p & 8).
 *   Decision:  found = sw >= min_support && (seen || !guarded) && !(edge_guard && (edge_prev || edge_cur)).  The blend is unchanged, over the taps of sw.
 *   d_status (optional, one u8 per pixel): bit 0 projected; bit 1 found; bit 2 found_geometry; bit 3 edge_prev; bit 4 edge_cur.  Bits 1 .. 4 are 0 for a pixel that
 *     is not both projected and filterable; bits 3 and 4 are reported whatever edge_guard says (edge_guard 0 only keeps them out of the decision).  "Lost to shading"
 *     is bit 2 without bit 1; of those, "lost to an edge guard" are the ones whose taps alone (the same call with edge_guard 0) would have found history.
 *   d_prev_xy, d_weight and d_prev_position are as in the stage above (d_prev_position needs a motion).
 * With flags of one sun state throughout and a history whose word 15 is 0, the stage is the one above bit for bit (word 15 of `next` aside).
 * WHAT IS STILL NOT FOLLOWED: a Sun that moves in the model frame (every surface's radiance changes with the cosine while no bit flips); indirect light from a moved
 * body (a lit body brightens the station next to it); view-dependent materials (metal, glass).  alpha_min remains the guard against those.  A silhouette pixel's
 * bilinear footprint still mixes partial background coverage, as in TEMPORAL ACCUMULATION.
 *
 * dsrt_denoise_temporal_shaded: dsrt_denoise_temporal_bodies with `shading` after `motion` and d_status after d_prev_position; `motion` may be NULL.  Stream order,
 *   waiting, working memory and "needs no scene" are unchanged.  DSRT_ERR_INVALID: what dsrt_denoise_temporal_bodies refuses (a NULL motion excepted); a NULL shading
 *   or NULL flags; edge_guard outside {0, 1}; d_prev_position without a motion; flags or d_status overlapping an output or each other, d_status overlapping an input
 *   or the previous history.  A refused call touches no buffer.
 * dsrt_denoise_temporal_shaded_to_host: the same from HOST buffers into HOST buffers (flags and status too), synchronously.
 * dsrt_ctx_set_temporal_shading / dsrt_ctx_temporal_shading: the switch of the convenience form, per context (a clone has its own, off): 0 off (the default), 1 the
 *   tap test only (edge_guard 0), 2 with the edge guards; another mode is DSRT_ERR_INVALID.  On: dsrt_render_denoised_temporal_to_host asks its G-buffer for flags as
 *   well (that channel traces the shadow rays) and runs the stage above, with the motion when dsrt_ctx_set_temporal_bodies is on and the scene has bodies, without one
 *   otherwise.  The result is exactly the explicit chain of dsrt_denoise_temporal_shaded calls.  The switch may change between two frames of a sequence.
 */
typedef struct DsrtTemporalShading {
    const uint8_t* flags;       /* DEVICE (HOST in the host form), one per pixel: the current G-buffer's flags channel */
    int edge_guard;             /* 0: the tap test only; 1: history next to a sun-state edge of either frame is voided too */
} DsrtTemporalShading;
int  dsrt_denoise_temporal_shaded(DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtAccum* acc, int samples_done, const uint32_t* d_n, const DsrtDenoiseGuides* guides,
                                  const DsrtBodyMotion* motion /* NULL: static scene */, const DsrtTemporalShading* shading, const GPUCamera* prev_camera /* HOST */,
                                  const float* d_history_prev, float* d_history_next, const DsrtTemporal* temporal, const DsrtDenoise* params, uint8_t* d_rgb8, float* d_f32,
                                  float* d_linear, float* d_var, float* d_prev_xy, float* d_weight, float* d_prev_position, uint8_t* d_status, void* stream);
int  dsrt_denoise_temporal_shaded_to_host(DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtAccum* h_acc, int samples_done, const uint32_t* h_n,
                                          const DsrtDenoiseGuides* h_guides, const DsrtBodyMotion* motion, const DsrtTemporalShading* shading, const GPUCamera* prev_camera,
                                          const float* h_history_prev, float* h_history_next, const DsrtTemporal* temporal, const DsrtDenoise* params, uint8_t* h_rgb8,
                                          float* h_f32, float* h_linear, float* h_var, float* h_prev_xy, float* h_weight, float* h_prev_position, uint8_t* h_status);
int  dsrt_ctx_set_temporal_shading(DsrtContext* ctx, int mode);
int  dsrt_ctx_temporal_shading(const DsrtContext* ctx);

/*
 * UPSCALER (on top of the DENOISER and the G-BUFFER): a full-resolution frame out of a low-resolution render.  Joint bilateral upsampling (Kopf et al. 2007) whose
 * guides are GROUND TRUTH at the output resolution: the Monte-Carlo radiance is rendered (and denoised) at w x h, the G-buffer -- normal, position, albedo, range and
 * the sun-visibility bit of every pixel-centre ray, a few milliseconds at 4K -- at W x H, and every output pixel gathers the 4 x 4 low-resolution pixels around it
 * that lie on its own surface, in its own material and on its own side of the sun's shadow edge.  Silhouettes, creases, material edges and the hard shadows of the
 * delta light stay at the output resolution.  Like the denoiser it uses correctly rounded fp32 operations only: tests/_upscale_model.py reproduces every bit.
 *
 * THE ARITHMETIC.  All fp32; every operation one correctly rounded IEEE operation, never contracted, in the order written; dot is the DENOISER's; / and floorf are
 * the IEEE ones; the constants are float literals.
 *   Inputs.  Low resolution w x h: linear colour c (3 floats per pixel: the denoiser's d_linear, or a resolved mean), optionally its variance v, the guides N, X, A,
 *     range, optionally flags (the G-buffer's uint8 channel).  Output resolution W x H, W >= w and H >= h (no integer factor required): the same guides from a G-buffer
 *     of the SAME camera pose and field of view.  The camera's lower_left_corner / horizontal / vertical do not depend on the image size, so dsrt_render_gbuffer with
 *     desc->width, height = W, H and the context's unchanged camera is that G-buffer.
 *   Per output pixel P = (X, Y) (Y the buffer row, 0 the top row), R = range_hi[P]:
 *     !(R <= FLT_MAX) (a miss, or a NaN): c' = +0, v' = +0, support = +0 -- space stays black and the silhouette is the full-resolution G-buffer's.  Otherwise
 *     the position in the low-resolution buffer -- the G-buffer's pixel-centre ray parameter u = (x + 0.5) / (W - 1) mapped from one raster to the other:
 *       fx  = (((float)X + 0.5f) / (float)(W-1)) * (float)(w-1) - 0.5f
 *       fyk = (((float)(H-1-Y) + 0.5f) / (float)(H-1)) * (float)(h-1) - 0.5f
 *       fy  = (float)(h-1) - fyk
 *       x0  = (int)floorf(fx);   y0 = (int)floorf(fy)
 *     Taps qy = y0-1 .. y0+2 (outer), qx = x0-1 .. x0+2 (inner); a tap outside the low-resolution image is skipped.  Spatial weight, a tent of radius 2 (the sixteen
 *     weights sum to 4 in exact arithmetic):
 *       bx = fmaxf(1.0f - 0.5f*fabsf((float)qx - fx), 0.0f);   by likewise with qy and fy;   b = bx*by
 *     LEVEL 1 (guided).  A tap is also skipped when !(range_q <= FLT_MAX), or -- with use_sun != 0 and both flags arrays given -- when
 *     ((flags_q ^ flags_P) & DSRT_GB_SUN_VISIBLE) != 0.  For the other taps
 *       wn  = fmaxf(dot(N_P, N_q), 0.0f);   normal_power_log2 times: wn = wn*wn
 *       D   = X_q - X_P;   ez = fabsf(dot(N_P, D)) / (sigma_z * R)
 *       da  = A_q - A_P;   ea2 = dot(da, da) / (sigma_a*sigma_a)
 *       wt  = (b * wn) / ((1.0f + ez*ez) * (1.0f + ea2))
 *       sw += wt;   sc.k += wt*c_q.k;   sv.k += (wt*wt)*v_q.k                          (k = r, g, b; all sums start at +0.0f)
 *     sw > 0:  c'.k = sc.k/sw,  v'.k = sv.k/(sw*sw),  support = sw.
 *     LEVEL 2 (fallback, when !(sw > 0)).  The same loop and the same quotients over EVERY tap inside the image with wt = b alone -- low-resolution miss pixels count
 *     too: a partly covered low-resolution pixel still carries light -- and support = +0.  At least one tap is always inside the image with positive weight:
 *     fx lies in (-0.5, w-1] (X = 0 gives 0.5 (w-1)/(W-1) - 0.5 > -0.5; X = W-1 gives (w-1) - 0.5 (1 - (w-1)/(W-1)) <= w-1), so either x0 >= 0 and tap x0 is
 *     a column of the image at a distance below 1, weight above 0.5, or x0 = -1 and tap x0+1 = 0 is at a distance below 0.5, weight above 0.75; fy lies in
 *     [0, h-0.5) and tap y0 is a row of the image, weight above 0.5; a few units in the last place of fx or fy change neither.  So level 2 never divides by zero.
 *   Outputs.  d_linear = c', d_var = v', d_support = support (one float per pixel: 0 exactly where the miss rule or level 2 applied); d_rgb8 and d_f32 are
 *     dsrt_resolve_accumulated's tone map and 8-bit store applied to c' (desc->gamma; desc->math_mode chooses powf as it does there).
 * DELIBERATELY NOT IN: albedo demodulation (divide by the low-resolution albedo, multiply by the full-resolution one).  Every sample is clamped to [0,1] before it is
 * summed (the reference's src/gpu_render.cu:935) and the sun's radiance is 1e5, so a sunlit pixel's mean is NOT albedo times irradiance, and demodulating it is wrong.
 * The albedo is an edge-stopping guide only.
 * Guides must be finite wherever `range` is finite; the call does not check.
 *
 * dsrt_upscale_guided: desc gives W, H (width, height), gamma and math_mode (rng_mode must be 1 like everywhere in this family; the sampling fields are ignored);
 *   lo / hi are the guides at w x h and W x H (flags optional in each); at least one of d_rgb8 (bytes, W*H*3), d_f32, d_linear, d_var (floats, W*H*3) and d_support
 *   (floats, W*H).  Asynchronous on `stream`; like dsrt_denoise_accumulated it waits for the context's previous launch, the next launch waits for it, it needs no scene,
 *   and the context's camera, sun and render buffers are left as they were.  Inputs are read only.  Working memory (80 bytes per LOW-resolution pixel: five 16-byte
 *   records {c, range}, {v, flags}, {N}, {X}, {A}) belongs to the context: allocated on first use, grown for a larger frame, freed by dsrt_ctx_destroy.
 *   DSRT_ERR_INVALID: what the denoiser refuses of desc (rng_mode != 1, math_mode not 0 or 1, shard_count > 1, W or H < 2, 2^31 pixels); lo_width or lo_height < 2;
 *   W < lo_width or H < lo_height; a NULL ctx, desc, colour, guide struct, normal / position / albedo / range channel or params; normal_power_log2 outside [0, 8]; a
 *   sigma that is not > 0 (NaN is refused); no output; d_var without d_lo_var; a pointer not aligned to its element; an output range that overlaps an input range or
 *   another output.  A refused call touches no buffer.
 * dsrt_upscale_guided_to_host: the same from HOST buffers into HOST buffers, synchronously.
 * dsrt_render_upscaled_to_host: the convenience form.  lo_desc plans the low-resolution frame (w x h, spp >= 2, rng_mode 1); in order: lo_desc->spp samples with second
 *   moments at w x h; the G-buffer at w x h (normal, position, albedo, range, flags); dsrt_denoise_accumulated with `denoise` (NULL = the defaults with iterations 0:
 *   the plain mean and variance); the G-buffer at out_width x out_height; dsrt_upscale_guided.  The result is exactly that chain of five calls.  h_lo_rgb8 (optional,
 *   w*h*3 bytes) receives the low-resolution image of the third step: dsrt_render_denoised_to_host's.  DSRT_ERR_NO_SCENE before an upload.  stats (optional): the
 *   accumulate launch's.
 * dsrt_upscale_defaults: the denoiser's where the terms are the denoiser's -- normal_power_log2 5, sigma_z 0.01, sigma_a 0.1 -- and use_sun 1.
 *   The values stayed where they started.  Measured on the CPU model (tests/test_upscale_host.py), MSE over the output pixels that hit against
 *   256 spp at the output size, relative to bilinear interpolation of the same denoised low-resolution image: station_near 100 x 56 -> 200 x 112 at 16 spp 0.775 (0.880
 *   with use_sun 0), textured 48 x 32 -> 96 x 64 at 8 spp 0.695 (1.454 with use_sun 0: without the bit the guides concentrate the weight on fewer taps across a shadow
 *   edge they cannot see, and the result is worse than no guides at all -- use_sun 1 is what makes the default work, and a caller without the flags channel should know).
 *   Against the same sample budget rendered natively (spp / 4 at the output size, denoised) the upscaled frame's error is 1.70 times on the station, whose trusses are
 *   thinner than a low-resolution pixel, and 0.80 times in the textured room.  On an MI355X the kernel takes 74 us at 960 x 540 -> 1920 x 1080 and 270 us at
 *   1920 x 1080 -> 3840 x 2160 (a third of one a-trous iteration at the output size), the call 0.14 and 0.37 ms.
 */
typedef struct DsrtUpscaleGuides {   /* DEVICE (HOST for _to_host) buffers, one raster's width*height elements, image order: channels of DsrtGBuffer */
    const float*   normal;           /* x3 */
    const float*   position;         /* x3 */
    const float*   albedo;           /* x3 */
    const float*   range;            /* x1, +inf on a miss */
    const uint8_t* flags;            /* optional: DSRT_GB_*; only DSRT_GB_SUN_VISIBLE is looked at */
} DsrtUpscaleGuides;
typedef struct DsrtUpscale { int normal_power_log2; float sigma_z, sigma_a; int use_sun; } DsrtUpscale;
void dsrt_upscale_defaults(DsrtUpscale* out);
int  dsrt_upscale_guided(DsrtContext* ctx, const DsrtRenderDesc* desc /* width, height = W, H; gamma; math_mode */, int lo_width, int lo_height, const float* d_lo_linear,
                         const float* d_lo_var /* optional */, const DsrtUpscaleGuides* lo, const DsrtUpscaleGuides* hi, const DsrtUpscale* params, uint8_t* d_rgb8,
                         float* d_f32, float* d_linear, float* d_var, float* d_support, void* stream);
int  dsrt_upscale_guided_to_host(DsrtContext* ctx, const DsrtRenderDesc* desc, int lo_width, int lo_height, const float* h_lo_linear, const float* h_lo_var,
                                 const DsrtUpscaleGuides* h_lo, const DsrtUpscaleGuides* h_hi, const DsrtUpscale* params, uint8_t* h_rgb8, float* h_f32, float* h_linear,
                                 float* h_var, float* h_support);
int  dsrt_render_upscaled_to_host(DsrtContext* ctx, const DsrtRenderDesc* lo_desc, int out_width, int out_height, const DsrtDenoise* denoise /* NULL = iterations 0 */,
                                  const DsrtUpscale* params, uint8_t* h_rgb8, float* h_f32, float* h_linear, float* h_var, uint8_t* h_lo_rgb8 /* optional, w*h*3 */,
                                  DsrtStats* stats);

/*
 * COVERAGE-AWARE UPSCALER (dsrt_upscale_guided_coverage; on top of the UPSCALER and COVERAGE).  A low-resolution pixel that a truss crosses holds alpha x (the
 * radiance of the truss), alpha the share of its samples that hit: its mean mixes structure and space, and no guide can unmix it.  A DIAGONAL coverage pass at each
 * raster can: take the low-resolution mean / alpha, upsample it guided by full-resolution ground truth, and multiply by a full-resolution alpha.  The guides lo / hi
 * are meant to be the `rep` channels of the same passes, so `range` is finite wherever any sub-sample hit: an output pixel whose centre ray misses but which a truss
 * crosses is no longer black, and a low-resolution pixel whose centre ray misses is a tap.  Plain G-buffer channels are legal too.  tests/_upscale_coverage_model.py
 * reproduces every bit.
 *
 * THE ARITHMETIC.  All fp32; every operation one correctly rounded IEEE operation, never contracted, in the order written.  "as UPSCALER" is the arithmetic above,
 * word for word.
 *   Inputs beyond UPSCALER's: alpha_lo (w x h floats), alpha_hi (W x H floats), both the `alpha` of a DIAGONAL coverage pass; alpha_min in (0, 1].
 *   Per output pixel P, R = range_hi[P], aP = alpha_hi[P]:
 *     LEVEL 0.  !(R <= FLT_MAX) || !(aP > 0.0f) (a NaN alpha included): c' = v' = support = +0.  Otherwise fx, fy, x0, y0, the 4 x 4 taps, their order (qy outer,
 *     qx inner) and the tent b are as UPSCALER.
 *     Per tap q, a = alpha_lo[q]: the tap is USABLE iff a >= alpha_min (a NaN alpha is not).  For a usable tap
 *       u.k = c_q.k / a;   aa = a * a;   vu.k = v_q.k / aa
 *     LEVEL 1 (guided, unmixed).  Skipped: a tap outside the image, a tap that is not usable, a tap with !(range_q <= FLT_MAX), a tap on the other side of the sun
 *     bit (UPSCALER's use_sun rule).  For the others wn, ez, ea2 as UPSCALER and
 *       wt = ((b * wn) * a) / ((1.0f + ez*ez) * (1.0f + ea2))          -- the factor a weighs a tap by the share of its samples that landed on structure
 *       sw += wt;   sc.k += wt*u.k;   sv.k += (wt*wt)*vu.k
 *     sw > 0:  c'.k = (sc.k/sw) * aP,  v'.k = (sv.k/(sw*sw)) * (aP*aP),  support = sw.
 *     LEVEL 2 (when !(sw > 0)).  The same loop over every usable tap inside the image, no range or sun test, wt = b * a; the same quotients and the same
 *     multiplication by aP and aP*aP; support = +0.
 *     LEVEL 3 (when still !(sw > 0)).  UPSCALER's level 2 exactly: every tap inside the image, wt = b, the mixed c_q and v_q, and no multiplication by aP; it never
 *     divides by zero, by the argument above.  support = +0.
 *   Outputs.  UPSCALER's, with its tone map and 8-bit store applied to c', and d_level (optional, one byte per pixel): 0, 1, 2 or 3, the level that produced the pixel.
 *   TWO IDENTITIES.  With both alpha pointers NULL the call is dsrt_upscale_guided bit for bit (alpha_min is then only checked, and d_level must be NULL: the plain
 *   upscaler has no such output).  With both alphas 1.0f everywhere and any legal alpha_min the results are dsrt_upscale_guided's bit for bit: x / 1, x * 1 and
 *   (b * wn) * 1 are exact, every tap is usable, and level 2 is then the old level 2 (its sw is positive, so level 3 is never reached).
 *
 * dsrt_upscale_guided_coverage: dsrt_upscale_guided's envelope, stream ordering and working-memory ownership.  Working memory stays 80 bytes per low-resolution
 *   pixel: alpha_lo rides in the spare word of the normal record, {N, alpha} (the {c, range} record that decides whether a tap counts has no spare word).
 *   DSRT_ERR_INVALID: everything dsrt_upscale_guided refuses (d_level counts as an output); exactly one alpha pointer given; alpha_min not in (0, 1] (NaN is
 *   refused); d_level without the alphas; a misaligned alpha pointer; d_level or an alpha overlapping an output.  A refused call touches no buffer.
 * dsrt_upscale_guided_coverage_to_host: the same from HOST buffers into HOST buffers, synchronously.
 * dsrt_render_upscaled_coverage_to_host: the convenience form, exactly this chain of calls, in order: lo_desc->spp samples with second moments at w x h; a DIAGONAL
 *   coverage pass at w x h (alpha and rep: normal, position, albedo, range, flags); dsrt_denoise_accumulated_coverage with those (denoise NULL = iterations 0); a
 *   DIAGONAL coverage pass at out_width x out_height; dsrt_upscale_guided_coverage.  cov_lo / cov_hi NULL = dsrt_coverage_defaults; a GRID pattern is refused, as
 *   dsrt_render_denoised_coverage_to_host refuses it.  The denoiser and the upscaler share the one alpha_min.  h_lo_rgb8 (optional, w*h*3 bytes): the third step's
 *   image; h_alpha_hi (optional, out_width*out_height floats): the fourth step's alpha.  DSRT_ERR_NO_SCENE before an upload.  stats (optional): the accumulate launch's.
 * dsrt_upscale_coverage_alpha_min: the default alpha_min of this chain, 1/8 -- not the denoiser's 1/16: measured below, 1/8 is the best of {1/64, 1/16, 1/8, 1/4} over
 *   the covered pixels and over the whole frame on both scenes (by 0.7 % and 0.4 % over 1/16).
 *   Measured on the CPU model (tests/test_upscale_coverage_host.py): DIAGONAL 64 at both rasters, the coverage-aware denoiser in front, MSE
 *   against 256 spp at the output size under another seed; "plain" is dsrt_upscale_guided's chain, "native" the same sample budget (spp / 4) at the output size,
 *   coverage-denoised; sets: partial = 0 < alpha_hi < 1, centre misses = the centre ray misses and alpha_hi > 0 (dsrt_upscale_guided writes these black), covered =
 *   alpha_hi > 0.  MSE plain / native / this chain with alpha_min 1/64, 1/16, 1/8, 1/4 / with 1/8 and DIAGONAL 16 at the output raster:
 *     station_near 100 x 56 -> 200 x 112, 16 spp
 *       partial        2789 px: 1.312e-2 / 3.99e-3 / 5.23e-3, 3.49e-3, 3.31e-3, 3.98e-3 / 3.40e-3
 *       centre misses  1529 px: 9.70e-3 / 2.13e-3 / 2.00e-3, 1.70e-3, 1.70e-3, 1.82e-3 / 1.68e-3
 *       covered        9665 px: 8.831e-3 / 4.199e-3 / 6.054e-3, 5.541e-3, 5.500e-3, 5.713e-3 / 5.470e-3         levels 0..3 at 1/8: 12735, 9542, 123, 0
 *     textured 48 x 32 -> 96 x 64, 8 spp
 *       partial         238 px: 4.743e-2 / 8.29e-3 / 3.00e-4, 2.80e-4, 2.64e-4, 2.99e-4 / 4.30e-4
 *       centre misses   141 px: 4.781e-2 / 1.001e-2 / 7.77e-5, 7.56e-5, 7.37e-5, 7.27e-5 / 2.29e-4
 *       covered        3203 px: 8.896e-3 / 8.123e-3 / 4.887e-3, 4.874e-3, 4.853e-3, 4.853e-3 / 4.874e-3         levels 0..3 at 1/8: 2941, 3203, 0, 0
 *   Over the covered pixels this chain has 0.62 (station) and 0.55 (room) of the plain chain's error, and 1.31 and 0.60 of the native frame's: the successor of
 *   UPSCALER's 1.70, which is the plain chain against the plain native frame over the same pixels.  Measured on an MI355X (GPU probe, tools/upscale_probe.py): the
 *   gather kernel takes 102 us at 960 x 540 -> 1920 x 1080 and 363 us at 1920 x 1080 -> 3840 x 2160, 1.36 and 1.34 times dsrt_upscale_guided's; what the form costs
 *   is the output raster's coverage pass, 7.9 / 23.9 ms at 1080p and 25.8 / 86.4 ms at 4K for DIAGONAL 16 / 64.  With 64 sub-samples the whole frame is slower than
 *   the native frame of the same sample budget; 16 is the recommended count for cov_hi.
 */
float dsrt_upscale_coverage_alpha_min(void);
int  dsrt_upscale_guided_coverage(DsrtContext* ctx, const DsrtRenderDesc* desc, int lo_width, int lo_height, const float* d_lo_linear, const float* d_lo_var /* optional */,
                                  const DsrtUpscaleGuides* lo, const DsrtUpscaleGuides* hi, const float* d_lo_alpha, const float* d_hi_alpha, float alpha_min,
                                  const DsrtUpscale* params, uint8_t* d_rgb8, float* d_f32, float* d_linear, float* d_var, float* d_support, uint8_t* d_level, void* stream);
int  dsrt_upscale_guided_coverage_to_host(DsrtContext* ctx, const DsrtRenderDesc* desc, int lo_width, int lo_height, const float* h_lo_linear, const float* h_lo_var,
                                          const DsrtUpscaleGuides* h_lo, const DsrtUpscaleGuides* h_hi, const float* h_lo_alpha, const float* h_hi_alpha, float alpha_min,
                                          const DsrtUpscale* params, uint8_t* h_rgb8, float* h_f32, float* h_linear, float* h_var, float* h_support, uint8_t* h_level);
int  dsrt_render_upscaled_coverage_to_host(DsrtContext* ctx, const DsrtRenderDesc* lo_desc, int out_width, int out_height, const DsrtCoverageDesc* cov_lo /* NULL = defaults */,
                                           const DsrtCoverageDesc* cov_hi /* NULL = defaults */, float alpha_min, const DsrtDenoise* denoise /* NULL = iterations 0 */,
                                           const DsrtUpscale* params, uint8_t* h_rgb8, float* h_f32, float* h_linear, float* h_var, uint8_t* h_lo_rgb8 /* optional, w*h*3 */,
                                           float* h_alpha_hi /* optional, W*H */, DsrtStats* stats);

/*
 * SENSOR MODEL (after the DENOISER or the UPSCALER): the clean linear frame as a navigation camera would have delivered it -- optical blur, photon shot noise, read
 * noise, fixed-pattern noise, full-well saturation and an ADC of 8 to 16 bits -- as a REPRODUCIBLE raw frame of DN (digital numbers, the ADC's output counts).  The
 * degradation acts on linear signal, which is why it belongs here and not on the tone-mapped 8-bit image; and the noise is counter-based Philox keyed by pixel, plane
 * and frame, so the same seed and frame index give the same DN on any GPU, under any launch shape, and in the CPU model: tests/_sensor_model.py reproduces every bit.
 * A dataset can be regenerated, and a failure traced to a pixel.
 * WHAT THE INPUT IS.  Every sample is clamped to [0, 1] before it is summed (the reference's src/gpu_render.cu:935), so the linear frame -- d_linear of the denoiser
 * and the upscalers -- is an exposure-normalised signal, not radiance: 1.0 is "the exposure's white".  gain_e maps signal 1.0 to electrons (full well x exposure).
 * Glare from a sunlit panel, blooming and anything else that needs radiance above white is therefore not representable.
 *
 * THE ARITHMETIC.  All fp32; every operation one correctly rounded IEEE operation, never contracted, in the order written; sqrtf, / and floorf are the IEEE ones;
 * fmaxf and fminf return the other operand when one is a NaN; the constants are float literals.
 *   Let C = 1 (mono != 0) or 3, and r = (psf_size - 1) / 2.  For plane k (0 .. C-1) of pixel P = (x, y), y the buffer row, 0 the top row:
 *   1. Input plane.  Colour: c_k is input channel k.  Mono: c = (0.2126f*r + 0.7152f*g) + 0.0722f*b of the input pixel -- the luminance is taken BEFORE the blur.
 *   2. Blur, a true convolution: the image of a point source is the PSF itself, not its mirror image.
 *        s = +0.0f;  for ky = -r .. r (outer), kx = -r .. r (inner): a tap with (x+kx, y+ky) outside the image is skipped (space is black); otherwise
 *        s = s + psf[(r-ky)*psf_size + (r-kx)] * c(x+kx, y+ky)
 *      One accumulator per plane; nothing is reassociated.  psf == NULL is psf_size = 1 with the tap 1.0f, bit for bit (so an input of -0.0f gives s = +0.0f).
 *   3. Gaussian-like draws, one Philox4x32-10 block each (the generator of rng_mode 1): key = (seed's low word, seed's high word),
 *        counter = (y*W + x,  k + 4*kind,  frame_word,  0x53454E53)
 *      kind 0 is the temporal draw z0, with frame_word = frame; kind 1 is the PRNU draw z1 and kind 2 the DSNU draw z2, both with frame_word = 0: the fixed
 *      pattern does not depend on `frame`.  With S the integer sum of the eight 16-bit halves of the block's four output words,
 *        z = ((float)S - 262140.0f) * kInvSigma,      kInvSigma = 0x1.3988e2p-16f
 *      the fp32 value nearest 1/sqrt(2863311530); 2863311530 = 8 (2^32 - 1) / 12 is the variance of S and 262140 = 8 x 65535 / 2 its mean.  This is an
 *      Irwin-Hall sum of eight uniform terms: unit variance, excess kurtosis -0.15, tails cut at +-4.9 sigma.  (The library has no deterministic logf, and a
 *      Box-Muller transform would need one.)  A draw whose coefficient is zero is NOT generated and counts as +0.0f: z1 when prnu == 0, z2 when dsnu_e == 0, z0
 *      when noise == 0.
 *   4. Electrons.
 *        e  = s * gain_e
 *        e  = e * (1.0f + prnu*z1)
 *        d  = fmaxf(dark_e + dsnu_e*z2, 0.0f)
 *        m  = fmaxf(e, 0.0f) + d
 *        sg = sqrtf(m + read_e*read_e)                  -- shot noise of variance m and read noise, as one Gaussian
 *        q  = fminf(m + sg*z0, full_well_e)
 *   5. ADC.
 *        v  = floorf((q / e_per_dn + offset_dn) + 0.5f)
 *        DN = 0 when !(v >= 0) (a NaN included), 2^bits - 1 when v > 2^bits - 1, (uint16_t)v otherwise.
 *   6. Outputs; at least one, and any subset gives the same bytes in each.
 *        d_dn      W*H*C uint16_t, interleaved like the input (mono: one per pixel)
 *        d_signal  W*H*C floats: the noise-free s of step 2, the blurred ground truth
 *        d_rgb8    always W*H*3 bytes: DN >> (bits - 8); a mono plane is written three times
 *
 * dsrt_sensor_apply: desc gives width and height and nothing else; d_linear is W*H*3 floats.  Asynchronous on `stream`; like dsrt_upscale_guided it waits for the
 *   context's previous launch, the next launch waits for it, it needs no scene, and the context's camera, sun and render buffers are left as they were.  The input is
 *   read only.  The taps are copied into a device buffer that belongs to the context (grown on demand, freed by dsrt_ctx_destroy) before the call returns; a call
 *   whose taps differ from the last call's waits on the host for the context's previous launch first, a call with the same taps uploads nothing.
 *   DSRT_ERR_INVALID: a NULL ctx, desc, input or params; W or H < 2, 2^31 pixels; with a psf, psf_size even or outside [1, 33], or a tap that is negative or not
 *   finite; gain_e, e_per_dn or full_well_e not > 0, prnu, dark_e, dsnu_e or read_e not >= 0 (NaN is refused by the same tests); offset_dn not finite; bits
 *   outside [8, 16]; no output; a pointer not aligned to its element; an output range that overlaps the input or another output.  A refused call touches no buffer.
 * dsrt_sensor_apply_to_host: the same from a HOST buffer into HOST buffers, synchronously.
 * dsrt_sensor_defaults: psf NULL (psf_size 0), mono 0, gain_e 20000, prnu 0, dark_e 0, dsnu_e 0, read_e 10, full_well_e 20000, e_per_dn 5, offset_dn 64, bits 12,
 *   noise 1, seed 1337, frame 0: white just fills the well, and the well just fills the 12-bit ADC above its offset.
 * dsrt_sensor_psf_gaussian: a host helper.  taps[size*size], row-major: exp(-(kx^2 + ky^2) / (2 sigma^2)) in double, divided by the double sum of the taps taken in
 *   row-major order, rounded to float.  A convenience: its bits are NOT part of the contract (exp is the C library's).  DSRT_ERR_INVALID: size even or outside
 *   [1, 33], sigma not > 0 or not finite, NULL taps.
 * dsrt_write_pnm16: a raw frame as a PNM file: P5 (channels 1) or P6 (channels 3), rows top-down, maxval = 2^bits - 1; two bytes per sample, most significant
 *   first, when maxval > 255 (one byte otherwise: the format's own rule).
 */
typedef struct DsrtSensor {
    const float* psf; int psf_size;   /* HOST pointer, psf_size x psf_size taps, row-major; psf_size odd, 1..33; NULL = no blur (psf_size is then ignored) */
    int   mono;                       /* 0: three planes r,g,b   1: one plane, luminance taken BEFORE the blur */
    float gain_e;                     /* electrons per unit of linear signal (full well x exposure) */
    float prnu;                       /* relative sigma of the per-pixel gain, fixed pattern */
    float dark_e, dsnu_e;             /* dark electrons per frame, and the sigma of their fixed pattern */
    float read_e;                     /* read noise, electrons rms */
    float full_well_e;                /* saturation, electrons */
    float e_per_dn, offset_dn; int bits;   /* ADC: bits in [8, 16] */
    int   noise;                      /* 0: the temporal draw z0 is +0 and no Philox word is generated for it */
    uint64_t seed; uint32_t frame;
} DsrtSensor;
void dsrt_sensor_defaults(DsrtSensor* out);
int  dsrt_sensor_psf_gaussian(float sigma, int size, float* taps);
int  dsrt_sensor_apply(DsrtContext* ctx, const DsrtRenderDesc* desc /* width, height only */, const float* d_linear /* W*H*3 */, const DsrtSensor* params, uint16_t* d_dn,
                       float* d_signal, uint8_t* d_rgb8, void* stream);
int  dsrt_sensor_apply_to_host(DsrtContext* ctx, const DsrtRenderDesc* desc, const float* h_linear, const DsrtSensor* params, uint16_t* h_dn, float* h_signal, uint8_t* h_rgb8);
int  dsrt_write_pnm16(const char* path, const uint16_t* dn, int width, int height, int channels /* 1 = P5, 3 = P6 */, int maxval);

/*
 * POINT SOURCES (before the SENSOR MODEL): a star field in the linear frame.  The renderer's sky is exactly black; a navigation camera's is not: stars are what a
 * star tracker and an attitude filter work on, they appear and vanish behind trusses and visiting vehicles, and they are the natural input of the sensor model's PSF.
 * This pass projects a catalogue of directions through the context's camera, tests each star against the resident scene, and deposits its flux into the frame with
 * bilinear weights; per star it returns the sub-pixel centroid and the visibility, which are the labels of a star-identification or attitude data set.  Like every
 * output of this library the result is REPRODUCIBLE: deposits are summed as integers, so the frame does not depend on the order of the stars or of the additions
 * (a float atomicAdd splat differs in its last bits from run to run), and tests/_stars_model.py reproduces every bit.
 *
 * INPUTS.  count stars, 0 <= count <= 2^22.  dir: count x 3 floats, directions in the MODEL frame towards the star (dsrt_pose_dirs_to_model takes inertial
 * directions there); they need not be unit vectors.  flux: count x 3 floats, linear signal x pixel, r g b: the total a star adds to the frame, in the units of the
 * linear frame.  The camera C is the context's current one and the scene the resident one, as for dsrt_render_gbuffer; W = desc->width, H = desc->height.
 *
 * THE ARITHMETIC.  All fp32; every operation one correctly rounded IEEE operation, never contracted, in the order written; fmaxf and fminf return the other operand
 * when one is a NaN; the constants are float literals.  Per star i, with D = dir_i:
 *   1. Projection: TEMPORAL ACCUMULATION's, verbatim, with D in place of X_p - C.origin -- a, b, cc, eu, ev, ew, hu, vv, k, s, t, fx, fy and its two "not
 *      projected" rules, !(k > 0) and the window (-1, W) x (-1, H) with both borders excluded.  A zero, NaN or infinite D falls out as not projected by those same tests and needs
 *      no rule of its own: D = 0 gives cc = 0 and k = ew / 0, which is -inf or NaN and fails k > 0, or +inf, and then a*k = 0 * inf is a NaN that reaches fx; a NaN
 *      in D reaches k, fx or fy; an infinite D gives a k that is NaN or zero, or products inf * 0 and sums inf - inf that are NaN -- and a NaN fx or fy fails the
 *      window.  A star behind the camera has cc >= 0 (ew is negative for every camera of dsrt_camera_look_at) and fails k > 0.
 *   2. Occlusion, when occlusion != 0, for projected stars only: blocked = the boolean of scene_hit(ray(C.origin, D), 0.001f, 1e9f) in its any-hit form on the
 *      REFERENCE tree -- exactly what dsrt_trace_rays answers in mode DSRT_TRACE_ANY for that ray, spheres and posed bodies included.
 *      visible = projected && !blocked; with occlusion == 0, visible = projected.
 *   3. Deposit, for visible stars: x0, y0, wx, wy, ox, oy, the four taps, their order and their weights bq are TEMPORAL ACCUMULATION's.  A tap outside the image is
 *      skipped: flux falls off the edge.  For each tap inside the image and each channel k:
 *        d = flux_k * bq;   q = fminf(fmaxf(d * 16777216.0f, 0.0f), 1099511627776.0f);   n = (uint64_t)q  (truncation);   A[pixel][k] += n
 *      A is an integer sum of quanta of 2^-24, hence independent of every order; with count <= 2^22 and a star touching a pixel at most once, A < 2^62.  Negative,
 *      NaN and sub-quantum deposits are 0; a deposit above 2^16 (q above 2^40) counts as 2^16.
 *   4. Resolve, per pixel and channel: layer = (float)A * 0x1p-24f -- the conversion rounds to nearest, ties to even; the scaling is exact -- and
 *      out = linear_in + layer.  A pixel no star touched has layer = +0.0f, so an input of -0.0f comes out as +0.0f.
 *   Outputs; each optional, at least one, and any subset gives the same bytes in each:
 *        layer        W*H*3 floats
 *        linear_out   W*H*3 floats; needs linear_in (W*H*3 floats, read only)
 *        xy           count x 2 floats: (fx, fy) when projected -- blocked or not -- else (+0, +0)
 *        status       count bytes: bit 0 projected, bit 1 visible, bit 2 projected and all four taps inside the image (x0 >= 0, x0+1 < W, y0 >= 0, y0+1 < H)
 *
 * dsrt_render_stars: desc gives width and height and nothing else.  It behaves as dsrt_render_gbuffer does: asynchronous on `stream` unless `stats` is given (then it
 *   waits, and kernel_ms is the pass's time); it waits for the context's previous launch and the next launch waits for it; camera, sun, scene and render buffers are
 *   left as they were; DSRT_ERR_NO_SCENE before an upload.  Working memory belongs to the context (grown on demand, freed by dsrt_ctx_destroy): count words for the
 *   list of projected stars, and -- only when layer or linear_out is asked for -- the accumulator A, W*H*3 uint64_t: 50 MB at 1920 x 1080, 200 MB at 3840 x 2160.
 *   It is cleared when it is allocated, and every call's resolve pass hands it back all zeros.  count == 0 is legal: the layer is zero and out = in + 0.
 *   DSRT_ERR_INVALID: a NULL ctx, desc, stars or out; W or H < 2, 2^31 pixels; count outside [0, 2^22]; a NULL dir or flux with count > 0; no output; linear_out
 *   without linear_in; a float pointer not 4-byte aligned; an output range that overlaps an input or another output.  A refused call touches no buffer.
 * dsrt_render_stars_to_host: the same from HOST buffers into HOST buffers, synchronously.
 * dsrt_stars_from_catalog: a host helper.  dir = (cos dec cos ra, cos dec sin ra, sin dec) as doubles in the frame the catalogue is given in -- the caller brings
 *   them into the model frame with dsrt_pose_dirs_to_model -- and flux = flux_mag0 * 10^(-0.4 mag) per channel, rounded to float.  Its bits are NOT part of the
 *   contract (sin, cos and pow are the C library's).  DSRT_ERR_INVALID: n < 0, a NULL array.
 * dsrt_stars_synthetic_catalog: n stars uniform on the sphere from a splitmix64 stream of `seed`, magnitudes in [mag_min, mag_max] with the sky's rough count law
 *   N(< m) ~ 10^(0.5 m).  A stand-in for a real catalogue; its bits are not part of the contract either.  DSRT_ERR_INVALID: n < 0, mag_min > mag_max or not finite, a NULL array.
 */
typedef struct DsrtStars {
    int count;                        /* 0 .. 2^22 */
    int occlusion;                    /* 0: every projected star is visible */
    const float* dir;                 /* count x 3, model frame, towards the star */
    const float* flux;                /* count x 3, r g b */
    const float* linear_in;           /* W*H*3, or NULL when linear_out is not asked for */
} DsrtStars;
typedef struct DsrtStarsOut { float* layer; float* linear_out; float* xy; uint8_t* status; } DsrtStarsOut;
int  dsrt_render_stars(DsrtContext* ctx, const DsrtRenderDesc* desc /* width, height only */, const DsrtStars* stars, const DsrtStarsOut* out, void* stream, DsrtStats* stats);
int  dsrt_render_stars_to_host(DsrtContext* ctx, const DsrtRenderDesc* desc, const DsrtStars* h_stars, const DsrtStarsOut* h_out, DsrtStats* stats);
int  dsrt_stars_from_catalog(int n, const double* ra_deg, const double* dec_deg, const double* mag, const float flux_mag0[3], double* world_dirs /* n x 3 */, float* flux /* n x 3 */);
int  dsrt_stars_synthetic_catalog(uint64_t seed, int n, double mag_min, double mag_max, double* ra_deg, double* dec_deg, double* mag);

/*
 * LENS MODEL (after POINT SOURCES, before the SENSOR MODEL): the pinhole frame as a real lens would have formed it -- Brown-Conrady distortion (fx, fy, cx, cy, k1, k2,
 * p1, p2, k3: what every calibration tool emits, OpenCV's meaning and order of terms) and a flat field that falls off towards the corners.  The warp acts on the LINEAR
 * frame, the same call warps every label with it (nearest: words are copied, so id planes, masks and range go through untouched), it returns the map it used, and like
 * every output of this library the result is REPRODUCIBLE: tests/_lens_model.py reproduces every bit.
 *
 * THE FRAMES.  The source is a pinhole frame of src_width x src_height pixels with intrinsics src_fx, src_fy, src_cx, src_cy: a point at normalised coordinates
 * (xu, yu) -- x to the right, y DOWN, depth 1 -- lies at pixel (xu*src_fx + src_cx, yu*src_fy + src_cy), pixel centres at integer coordinates, row 0 on top.  The output
 * is the distorted camera's frame, W = desc->width by H = desc->height, intrinsics fx, fy, cx, cy.  dsrt_lens_intrinsics_from_camera gives the library's own pinhole.
 *
 * THE ARITHMETIC.  All fp32; every operation one correctly rounded IEEE operation, never contracted, in the order and with the parentheses written; / and floorf are the
 * IEEE ones; fmaxf returns the other operand when one is a NaN; the constants are float literals.  Per output pixel (x, y):
 *   1. Normalise.    xd = ((float)x - cx) / fx;   yd = ((float)y - cy) / fy
 *   2. The forward model distort(xu, yu), stated once and used by steps 3 and 4 and by dsrt_lens_distort_points:
 *        xx = xu*xu;  yy = yu*yu;  xy = xu*yu;  r2 = xx + yy
 *        rad = 1.0f + r2*(k1 + r2*(k2 + r2*k3))
 *        dx  = (2.0f*p1)*xy + p2*(r2 + 2.0f*xx)
 *        dy  = p1*(r2 + 2.0f*yy) + (2.0f*p2)*xy
 *        distort = (xu*rad + dx,  yu*rad + dy)
 *   3. The inverse, by fixed-point steps: xu = xd, yu = yd; then EXACTLY 12 times, rad, dx, dy taken at the current (xu, yu) and both coordinates replaced together:
 *        xu = (xd - dx) / rad;   yu = (yd - dy) / rad
 *      There is no early exit: control flow is wave-uniform and the bits do not depend on a tolerance.
 *   4. The certificate.  (xr, yr) = distort(xu, yu);
 *        inverted = fabsf((xr - xd)*fx) <= 0x1p-6f && fabsf((yr - yd)*fy) <= 0x1p-6f        -- a NaN fails
 *      Beyond the fold-over radius of a strong barrel an output pixel has no preimage; the iteration then ends somewhere, and this test says so: the library reports
 *      it per pixel and does not guess.  A pixel that is not inverted has no source position and no taps.
 *   5. The source position.  sx = xu*src_fx + src_cx;  sy = yu*src_fy + src_cy.  The window, in float, before any conversion to an integer:
 *        in_window = sx > -3.0f && sx < (float)src_width + 2.0f && sy > -3.0f && sy < (float)src_height + 2.0f      -- a NaN fails
 *      Outside the window the pixel has no taps (no tap of any filter could lie inside the source).
 *   6. The taps, C = channels interleaved 32-bit words per pixel.  A tap (qx, qy) is INSIDE when 0 <= qx < src_width and 0 <= qy < src_height.
 *        nearest (filter 0):     the one tap (floorf(sx + 0.5f), floorf(sy + 0.5f)); inside: its C words are copied untouched; not inside: fill_bits in each.
 *        bilinear (filter 1):    x0 = floorf(sx), tx = sx - x0;  weights wx[0] = 1.0f - tx, wx[1] = tx for the columns x0, x0 + 1; wy[] likewise from sy.
 *        Catmull-Rom (filter 2): x0 = floorf(sx), t = sx - x0;  for the columns x0 - 1, x0, x0 + 1, x0 + 2
 *                                  wx[0] = (((-0.5f*t) + 1.0f)*t - 0.5f)*t        wx[1] = (((1.5f*t) - 2.5f)*t)*t + 1.0f
 *                                  wx[2] = (((-1.5f*t) + 2.0f)*t + 0.5f)*t        wx[3] = (((0.5f*t) - 0.5f)*t)*t              wy[] likewise from sy.
 *        Filters 1 and 2: acc_k = +0.0f per channel; rows outer (ascending), columns inner (ascending); for a tap inside,  acc_k = acc_k + (wy[j]*wx[i])*c_k.
 *        A tap that is not inside is skipped (space is black); nothing is renormalised and nothing is reassociated.
 *   7. Vignetting, filters 1 and 2 only (nearest copies words).  ru2 = xu*xu + yu*yu;
 *        g = 1.0f + ru2*(v1 + ru2*(v2 + ru2*v3));   with cos4 != 0:  q = 1.0f + ru2;  g = g / (q*q)      -- the natural cos^4(theta), ru2 = tan^2(theta)
 *        g = fmaxf(g, 0.0f);   out_k = acc_k * g;   with clamp_zero != 0:  out_k = fmaxf(out_k, 0.0f)       -- Catmull-Rom has negative lobes
 *   8. Outputs; each optional, at least one, and any subset gives the same bytes in each:
 *        image    W*H*C 32-bit words (floats for filters 1 and 2).  A pixel that is not inverted: +0.0f (filters 1, 2) or fill_bits (nearest) in every word.
 *                 An inverted pixel outside the window: acc = +0.0f through step 7 (filters 1, 2), fill_bits (nearest).
 *        src_xy   W*H*2 floats: (sx, sy) when inverted -- in the window or not -- else (+0, +0).  The ground-truth map with which a caller warps anything else.
 *        status   W*H bytes: bit 0 inverted, bit 1 at least one tap of the chosen filter inside the source, bit 2 all of them inside.
 *   With every coefficient zero and the source's own intrinsics, sx and sy are the pixel grid wherever (((float)x - cx)/fx)*fx + cx == x (always so for a power-of-two
 *   focal length), and the three filters return the source's words -- filters 1 and 2 with -0.0f as +0.0f, since the sum starts at +0.0f, and for finite sources.
 *
 * WHAT IT DOES NOT DO.  Stars deposited before the warp (dsrt_render_stars) are resampled with the frame: their centroid labels are exact -- dsrt_lens_distort_points
 * of the xy the star pass returned -- but their flux is not conserved, to the order of the local magnification and the filter's response.  A deposit at given
 * centroids AFTER the warp is not here yet.  Nor are a rolling shutter, chromatic aberration or fisheye (equidistant, Kannala-Brandt) models.
 *
 * dsrt_lens_apply: desc gives width and height (the OUTPUT's) and nothing else; d_src is src_width*src_height*channels words, read only.  Asynchronous on `stream`; like
 *   dsrt_sensor_apply it waits for the context's previous launch, the next launch waits for it, it needs no scene, and the context's camera, sun and render buffers
 *   are left as they were.  It has no working memory.
 *   DSRT_ERR_INVALID: a NULL ctx, desc, source, params or out; W, H, src_width or src_height < 2, 2^31 pixels in either frame; a focal length (fx, fy, src_fx,
 *   src_fy) not > 0 or not finite; a principal point or a coefficient (k1, k2, k3, p1, p2, v1, v2, v3) not finite; filter outside [0, 2], channels outside [1, 4],
 *   cos4 or clamp_zero not 0 or 1; no output; a word or float pointer not 4-byte aligned; an output range that overlaps the source or another output.  A refused
 *   call touches no buffer.  The context is the last thing looked at ("null context"), so every other refusal can be seen without a device.
 * dsrt_lens_apply_to_host: the same from a HOST buffer into HOST buffers, synchronously.
 * dsrt_lens_defaults: every size, intrinsic and coefficient 0 (the caller sets the two frames), cos4 0, filter 2, channels 3, clamp_zero 1, fill_bits 0.
 * dsrt_lens_distort_points: a HOST function, the exact forward direction in closed form, for labels.  xy_src: n x 2 floats, positions in the SOURCE frame in pixels
 *   (star centroids from dsrt_render_stars, the temporal stage's prev_xy, keypoints).  Per point, with the arithmetic pinned as above:
 *        xu = (px - src_cx) / src_fx;  yu = (py - src_cy) / src_fy;  (xr, yr) = distort(xu, yu);  out = (xr*fx + cx,  yr*fy + cy)
 *   ok (optional, n bytes) is 1 when the input and the result are finite; otherwise it is 0 and out is (+0, +0).  Sizes, filter and channels are not looked at.
 *   DSRT_ERR_INVALID: NULL params, xy_src or xy_out; n < 0; the focal lengths, principal points and k1 .. p2 as for dsrt_lens_apply.
 * dsrt_lens_intrinsics_from_camera: out = {fx, fy, cx, cy} of the library's own pinhole at W x H, derived from TEMPORAL ACCUMULATION's projection, with normalised
 *   coordinates xu = -a/cc, yu = b/cc of that projection's a, b, cc:  fx = -ew (W-1)/hu,  cx = -eu (W-1)/hu - 0.5,  fy = -ew (H-1)/vv,  cy = (H-1) + 0.5 + ev (H-1)/vv.
 *   (The renderer's u = (x + 0.5)/(W - 1) and its row flip put the principal point off (W-1)/2.)  Computed in double and rounded once; a convenience whose bits are
 *   NOT part of the contract.  DSRT_ERR_INVALID: a NULL argument, W or H < 2, a camera whose hu, vv or ew is zero or not finite.
 */
typedef struct DsrtLens {
    int   src_width, src_height;          /* the pinhole frame that is read */
    float src_fx, src_fy, src_cx, src_cy; /* its intrinsics, in pixels (pixel centres at integer coordinates, row 0 on top) */
    float fx, fy, cx, cy;                 /* the output (distorted) camera's intrinsics; output size = desc->width x desc->height */
    float k1, k2, k3, p1, p2;             /* Brown-Conrady, OpenCV's meaning and order of terms */
    float v1, v2, v3; int cos4;           /* vignetting: polynomial in tan^2(theta), optional natural cos^4 */
    int   filter;                         /* 0 nearest (labels: words are copied), 1 bilinear, 2 Catmull-Rom */
    int   channels;                       /* 1..4 interleaved 32-bit words per pixel */
    int   clamp_zero;                     /* filters 1, 2: fmaxf(result, 0) -- Catmull-Rom has negative lobes */
    uint32_t fill_bits;                   /* nearest: the word written where there is no source */
} DsrtLens;
typedef struct DsrtLensOut { void* image; float* src_xy; uint8_t* status; } DsrtLensOut;
#define DSRT_LENS_NEAREST  0
#define DSRT_LENS_BILINEAR 1
#define DSRT_LENS_CUBIC    2
#define DSRT_LENS_INVERTED 1u            /* the bits of DsrtLensOut.status */
#define DSRT_LENS_ANY_TAP  2u
#define DSRT_LENS_ALL_TAPS 4u
void dsrt_lens_defaults(DsrtLens* out);
int  dsrt_lens_apply(DsrtContext* ctx, const DsrtRenderDesc* desc /* width, height only */, const void* d_src, const DsrtLens* params, const DsrtLensOut* out, void* stream);
int  dsrt_lens_apply_to_host(DsrtContext* ctx, const DsrtRenderDesc* desc, const void* h_src, const DsrtLens* params, const DsrtLensOut* h_out);
int  dsrt_lens_distort_points(const DsrtLens* params, int n, const float* xy_src, float* xy_out, uint8_t* ok /* optional */);
int  dsrt_lens_intrinsics_from_camera(const GPUCamera* cam, int width, int height, float out[4]);

/* Root rank, after a gather: tile-major shards [shard][tile][tile*tile*3] -> image-order rgb8. */
int dsrt_deinterleave_tiles(DsrtContext* ctx, const DsrtRenderDesc* desc, const uint8_t* d_gathered, uint8_t* d_rgb8_image,
                            void* stream);
/* The same for the gather of SHARDED BATCH launches (dsrt_render_batch with shard_count > 1): d_gathered = the ranks' buffers one after another,
 * each holding its part of frame 0, of frame 1, ... (`frames` parts of rgb8_bytes_padded bytes); d_rgb8_images receives the `frames` whole images. */
int dsrt_deinterleave_batch(DsrtContext* ctx, const DsrtRenderDesc* desc, int frames, const uint8_t* d_gathered, uint8_t* d_rgb8_images, void* stream);

/* Convenience for hosts without their own device buffers: render the whole image into HOST memory. */
int dsrt_render_to_host(DsrtContext* ctx, const DsrtRenderDesc* desc, uint8_t* h_rgb8, float* h_f32, DsrtStats* stats);

/* Device evaluation of the shared deterministic math (tests): out[i] = f(x[i]) on the GPU;
 * fn 0 = sin, 1 = cos, 2 = pow(x[i], y).  Host pointers. */
int dsrt_selftest_math(DsrtContext* ctx, int fn, const float* x, float y, float* out, int n);

/* Device evaluation of the render kernel's own material / frame helpers (csrc/device_math.h: reflect, refract, scatter_metal,
 * scatter_dielectric, build_onb, schlick -- src/gpu_render.cu:112-118, 195-212, 603-661) on explicit inputs, for comparison with known
 * answers produced by the reference's host code (tests/golden/ref_matkat.json).  12 words in and 12 words out per case, host pointers;
 * the packing per `fn` (0..5) is documented at dsrt_devkat_kernel in csrc/render_kernel.hip. */
int dsrt_selftest_devkat(DsrtContext* ctx, int fn, const float* in12, float* out12, int n);

/* Device check that the kernel's stateless Philox4x32-10 equals rocRAND's engine: the first n 32-bit words of
 * (seed, subsequence, offset 0) from both.  Host pointers. */
int dsrt_selftest_philox(DsrtContext* ctx, uint64_t seed, uint64_t subsequence, int n, uint32_t* ours, uint32_t* rocrand_words);

/* SELFTEST: the scheduling pre-pass ("Pre-pass, probe, rng_mode 1, batch"; tests/_schedule_model.py is its CPU model).  Test hooks only:
 * nothing else calls them, and none changes what a launch does.
 *
 * dsrt_selftest_read_schedule: n_words (>= 1) 32-bit words from word first_word of one of the working buffers the context's LAST launch left, after waiting
 * for the device.  The range is checked against the buffer's ALLOCATED length (buffers only grow: words beyond what the last launch wrote are stale or
 * never written); a range outside it, an array no launch of this context has allocated yet, an unknown array and a null pointer are refused with
 * DSRT_ERR_INVALID and `out` is not touched.  With mine = tiles_this_shard of dsrt_shard_layout, pre_stride = mine + 64, and frame f of a batch (f = 0 for
 * a single frame) at f * pre_stride:
 *   array 0, tile_cost    [0, mine)      the cost words: bit 31 = at least one 8x8 block of the tile is not provably empty, low bits = pixels whose centre ray
 *                                        hits anything.  Not written by a DSRT_TUNE_NATURAL_ORDER launch.
 *                         mine + 32 ...  the sched words: [0] n_heavy, [1] n_live, [2] spread, [3] slices, [4] chunk_len (every launch writes them;
 *                                        a natural-order launch: mine, mine, 64, the host's slices and chunk_len)
 *                         mine + 40, 41  list_len: the lengths of the heavy and the light pixel list (dsrt_render_accumulate_masked only)
 *   array 1, tile_order   [0, n_live)    the local tiles in the order they are handed out, heavy part [0, n_heavy) first.  STALE after a
 *                                        DSRT_TUNE_NATURAL_ORDER launch (that launch has no order array); entries from n_live on are never written.
 *   array 2, tile_work    [0, mine)      meaningful only after a probe (rng_mode 0, spp >= 256, no DSRT_TUNE_NO_PROBE / NATURAL_ORDER): per local tile the most
 *                                        rays one of its pixels needed for the probe's 4 samples, capped at 255; 0 for a tile outside the heavy part.  After a
 *                                        batch: the LAST frame's probe.
 *   array 3, batch_table  24 words per entry, 2 * frames entries (dsrt_render_batch only): cam[12], sun_dir[3], item_end, order_base, n_heavy, n_live, slices,
 *                                        chunk_len, image_slot, 2 unused.  Entry f is the first eighth of frame f's heavy tiles, entry frames + f the rest.
 *   array 4, pixel_list   (dsrt_render_accumulate_masked only) [0, mine * tile^2): the heavy list from 0, the light list from n_heavy * tile^2, entries
 *                                        x | row << 16; then one word per 8x8 block of every live tile in order: its exclusive offset into the two lists run together.
 *
 * The three array kernels of the pre-pass on plain HOST arrays, with temporary device buffers of their own, as dsrt_selftest_math runs the math kernel:
 *   dsrt_selftest_tile_order    cost[n] (low bits <= tile^2) -> order[n] (entries the kernel does not write: 0xFFFFFFFF) and sched5[0..4]; n may be 0.
 *   dsrt_selftest_tile_reorder  work[n_work], order[n_order] (in place), sched5 (sched5[0] <= n_order heavy entries, each below n_work; sched5[2] < 64 = dealt).
 *   dsrt_selftest_batch_table   per frame 5 sched words sched_stride (>= 5) apart and an order_base -> table_words[2 * frames * 24] (cameras zero, image_slot f) and the
 *                               total of work items.  tt = pixels per tile.
 * Anything that would make a kernel read or write outside those arrays is refused with DSRT_ERR_INVALID before anything is launched. */
int dsrt_selftest_read_schedule(DsrtContext* ctx, int array, size_t first_word, size_t n_words, uint32_t* out);
int dsrt_selftest_tile_order(DsrtContext* ctx, const uint32_t* cost, int n, int tile, uint32_t items_per_pixel, uint32_t resident_lanes, int spp, uint32_t* order,
                             uint32_t* sched5);
int dsrt_selftest_tile_reorder(DsrtContext* ctx, const uint32_t* work, int n_work, uint32_t* order, int n_order, const uint32_t* sched5);
int dsrt_selftest_batch_table(DsrtContext* ctx, const uint32_t* sched, uint32_t sched_stride, uint32_t frames, uint32_t tt, int rng_mode, int spp, int light_chunk_len,
                              const uint32_t* order_base, uint32_t* table_words, uint32_t* total_items);

/* ===================================================================================== */
/* All GPUs of a node from ONE host process (the reference's main() is one process calling */
/* gpu_render_scene per frame, src/main.cpp:310-431; it has no multi-GPU code).           */
/* ===================================================================================== */
typedef struct DsrtMulti DsrtMulti;

/* `devices[r]` is the HIP device of rank r.  Distinct devices: an RCCL communicator is created over them (ncclCommInitAll).
 * Ranks that share a device (a one-GPU box: tests) get the same code path with the gather done by device-to-device copies --
 * RCCL refuses duplicate devices.  `frames_in_flight` (>= 1) is used by dsrt_multi_render_sequence only. */
int  dsrt_multi_create(const int* devices, int n, int frames_in_flight, DsrtMulti** out);
void dsrt_multi_destroy(DsrtMulti* m);
int  dsrt_multi_count(const DsrtMulti* m);
int  dsrt_multi_uses_rccl(const DsrtMulti* m);
/* Self-test: a one-rank RCCL communicator on `device` and one ncclGather of `bytes` bytes through it, checked.  All of the collective
 * path that can run on a single GPU. */
int  dsrt_selftest_rccl_gather(int device, size_t bytes);

/* Development switches (scheduling experiments of the A/B tools under tools/; the bits are listed in csrc/api_context.hip).  One process-wide word; its initial
 * value is the environment variable DSRT_EXPERIMENT, read ONCE in the first dsrt_device_count / dsrt_ctx_create call -- never per render.  Undefined bits are
 * refused (DSRT_ERR_INVALID) and a non-zero word is announced on stderr.  None changes an image byte; bit 27 replaces the optional FLOAT image of a counting
 * build by timing words.  Not for production hosts. */
int  dsrt_dev_set_experiment(uint32_t word);
/* Test hook for the bounds-checked kernel build: overwrites 32-bit word `word_index` of the context's resident node-record array (device_layout.h: 16 words per
 * record, words 12 and 13 are the child references) and returns the previous value in *old_value.  A checked render of a scene corrupted this way must come
 * back with DSRT_ERR_DEVICE_FLAG, not hang. */
int  dsrt_selftest_poke_node_word(DsrtContext* ctx, size_t word_index, uint32_t value, uint32_t* old_value);
/* Test hook, the read-only counterpart: n_words 32-bit words from word first_word of a resident array -- 0 the node records (`pairs`), 1 the triangle pair
 * records, 2 the shading records -- after waiting for the device.  first_word + n_words beyond the array is refused; with out = NULL only that is checked. */
int  dsrt_selftest_read_scene_words(DsrtContext* ctx, int array, size_t first_word, size_t n_words, uint32_t* out);
/* The scene (HOST pointers, reference layouts) is converted and made resident once per device. */
int  dsrt_multi_scene_upload(DsrtMulti* m, const GPUScene* host_scene);
/* ONE frame over all ranks: interleaved screen tiles (tile g -> rank g mod N), one ncclGather of the equal-sized compact
 * buffers to rank 0, de-interleave there, image (width*height*3, top row first) copied to `h_rgb8` (host).  desc's shard fields
 * are ignored.  Optional outputs: per-rank render time in ms (HIP events; N floats) and the wall time of the whole call. */
int  dsrt_multi_render_frame(DsrtMulti* m, const DsrtRenderDesc* desc, const GPUCamera* cam, const float sun_dir_model[3],
                             uint8_t* h_rgb8, float* kernel_ms_per_rank, double* seconds);
/* MANY frames of the resident scene (src/main.cpp's frame loop): every rank renders ITS interleaved tiles of EVERY frame as sharded batch
 * launches (dsrt_render_batch with a shard), nearest frames first, one gather per launch for all its frames and the de-interleave on rank 0.
 * cams[i] / sun_dirs[3 i ..] as from dsrt_camera_look_at / dsrt_pose_to_frame.  h_images may be NULL (timing only) or hold n_frames host
 * pointers (NULL entries are skipped). */
int  dsrt_multi_render_sequence(DsrtMulti* m, const DsrtRenderDesc* desc, const GPUCamera* cams, const float* sun_dirs, int n_frames,
                                uint8_t* const* h_images, double* seconds);

/* Calibration of the roofline the render kernel is measured against (bench.py): a kernel with the render
 * kernel's launch shape (256-thread workgroups, 4 waves per SIMD, grid = resident set) in which `live_lanes` of every 64 lanes gather
 * random aligned 64-byte records from a table of `table_bytes` bytes, `iters` records per lane, and do nothing else.
 *   mode 0: each lane reads its record as 4 x 16-byte loads (the render kernel's access shape)
 *   mode 1: the four lanes of a quad read one record per load instruction into an LDS tile (global_load_lds_dwordx4), 4 x ds_read_b128 back
 *   mode 2: as 1 through registers (global_load_dwordx4 + ds_write_b128)
 * dependent != 0: the next record index depends on the loaded data (a traversal step); pad_valu: dependent v_fma per record.
 * Returns the kernel time (HIP events) and the number of records gathered.  No reference interface: measurement only. */
int dsrt_microbench_gather(int device, int mode, int dependent, int live_lanes, int pad_valu, size_t table_bytes, int iters,
                           float* out_ms, double* out_records);

/* The other calibration: what a vector-ALU instruction costs to issue.  `waves_per_simd` (1..8) workgroups per CU (one wave per SIMD each) each
 * issue iters x 32 instructions from eight independent register streams: pattern 0 = the instruction of `kind` 32 times, 1 = alternating with
 * v_add_f32, 2 = in pairs between pairs of v_add_f32 (some kinds cost far more back to back), 3 = 16 of them then 16 v_add_f32, 4 / 5 = as 1 / 3
 * with v_pk_mul_f32 as the partner; only the lanes in `lane_mask` execute them.
 * Returns the kernel time (HIP events), the wave-instructions issued and the shader clock during the run (the waves' s_memtime against the
 * 100 MHz s_memrealtime): cycles per instruction per SIMD = SIMDs x clock x time / instructions.  dsrt_microbench_valu_kinds /
 * _kind_name enumerate the kinds.  No reference interface: measurement only. */
int dsrt_microbench_valu(int device, int kind, int pattern, int waves_per_simd, int iters, uint64_t lane_mask, float* out_ms, double* out_wave_instructions,
                         double* out_shader_clock_GHz);
int dsrt_microbench_valu_kinds(void);
const char* dsrt_microbench_valu_kind_name(int kind);

/* The third calibration: what this board's HBM delivers to a plain streaming copy -- a float4 grid-stride kernel (16 bytes per lane per access), `blocks_per_cu`
 * 256-thread workgroups per CU, `bytes` per buffer (take it far beyond the 256 MB Infinity Cache), `reps` launches back to back; `mode` 0 = copy, 1 = read only,
 * 2 = write only, 3 = copy with non-temporal loads and stores.  Returns the time (HIP events)
 * and the bytes moved (read + written).  The figure bench.py prints as extras.hbm_copy_GBps_measured, next to the 8 TB/s of the specification.
 * No reference interface: measurement only. */
int dsrt_microbench_copy(int device, int mode, size_t bytes, int blocks_per_cu, int reps, float* out_ms, double* out_bytes_moved);

/* ===================================================================================== */
/* Drop-in layer: the reference's own three entry points.                                */
/* ===================================================================================== */
/* src/gpu_render.cu:1037-1038, declared at its call site src/main.cpp:24-25.  `scene` holds DEVICE pointers.
 * Blocking; writes image_gpu.ppm into the CWD; failures print to stderr and return (no file).  math_mode 0 unless the environment variable
 * DSRT_MATH_MODE is 1 (the signature has no room for it): with it the file is, byte for byte, the one the reference's own gpu_render_scene
 * writes when its source is built for this GPU. */
void gpu_render_scene(const GPUScene* scene, int width, int height);

/* C forms of build_gpu_scene / free_gpu_scene (inc/gpu_scene_builder.h:72-73): the C++ overloads taking
 * hittable_list/camera/vec3 live in deep-space-ray-tracer_amd/host/scene_model.hpp and forward here. */
int  dsrt_build_gpu_scene(const DsrtHostScene* hs, const GPUCamera* cam, const float sun_dir_model[3], GPUScene* out);
void dsrt_free_gpu_scene(GPUScene* scene);

#ifdef __cplusplus
}
#endif
#endif /* DSRT_H */
