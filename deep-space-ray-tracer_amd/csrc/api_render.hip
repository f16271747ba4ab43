// api_render.hip -- a render launch in stages (plan, working buffers, one of three pre-passes, launch and resolve, stats) as render_impl, and the entry points
// that are nothing but such a launch: dsrt_render, dsrt_render_batch, their _to_host forms, the shard layout and the tile de-interleave.
// Calls the launchers of render_kernel.hip, schedule_kernel.hip and sample_set_kernel.hip, and api_context.hip (experiment_word); api_sample_sets.hip calls render_impl.
#include <algorithm>
#include <cmath>

#include "api_internal.h"

namespace dsrt {
const RenderLaunchers& render_launchers(bool device_libm) { return device_libm ? devlibm::compiled_render_launchers() : compiled_render_launchers(); }
}  // namespace dsrt

using namespace dsrt;

// ---- A render launch (dsrt_render, dsrt_render_batch, dsrt_render_accumulate), in stages: plan_render refuses or decides everything, without a HIP call;
// grow_render_buffers sizes the context's working buffers; one of the three pre-passes orders the tiles; launch_and_resolve; read_render_stats. ----
namespace {

constexpr size_t kListLenSched = 8;                          // masked accumulate launches: the lengths of the heavy and the light list (path_machine.h, LISTED) are words 8 and 9 of
                                                             // the pre-pass's sched block, next to the words every fetch reads anyway and away from the queue words' atomics
static_assert(4 + 2 * (size_t)kNumCounters <= kQueueLightWord, "counters overlap the second queue word");

struct Tiling { int tile, tiles_x, tiles_y, total, mine, padded; };
bool make_tiling(const DsrtRenderDesc& d, Tiling& t) {
    t.tile = d.tile_size > 0 ? d.tile_size : 8;
    if (t.tile % 8 != 0 || t.tile > 1024 || d.width < 2 || d.height < 2) return false;
    const int count = d.shard_count > 1 ? d.shard_count : 1;
    if (d.shard_rank < 0 || d.shard_rank >= count) return false;
    t.tiles_x = (d.width + t.tile - 1) / t.tile;
    t.tiles_y = (d.height + t.tile - 1) / t.tile;
    t.total = t.tiles_x * t.tiles_y;
    t.mine = (t.total - d.shard_rank + count - 1) / count;
    t.padded = (t.total + count - 1) / count;
    return true;
}

constexpr int kLdsStackEntries = 8;                      // LDS short-stack: 8 entries per lane (what fits beside the tree top and the continuation strip); deeper entries spill.
constexpr int kThreadsPerBlock = 64 * kWavesPerBlock;
constexpr int kProbeSpp = 4;          // x every pixel of the heavy tiles: 7 ms at 1080p, near frame.  (1, 2, 4 or 8 samples order the tiles equally well.)

enum class PrePass { Batch, Ordered, Natural };

struct RenderPlan {
    Tiling t;
    RenderArgs a;                     // complete but for what grow_render_buffers (accum_fixed of the context's own sums, spill, sched) and the pre-pass (tile order, batch table) add
    RenderVariant variant;
    bool device_libm;                 // DsrtRenderDesc.math_mode 1: which compilation of render_kernel.hip `rl` is, and the resolve's powf
    const RenderLaunchers* rl;
    PrePass pre;
    bool cull, probe;                 // the pre-pass removes provably empty tiles / re-sorts the heavy tiles by measured cost ...
    int probe_spp;                    // ... at this many samples per pixel
    bool own_sums;                    // rng_mode 1 of dsrt_render(_batch): the sums are the context's, zeroed before and resolved behind the launch
    int frames, chunks, chunk_len, blocks;
    size_t out_pixels, pre_stride;    // pre_stride, per frame: tile costs / order, then the sched words
    uint32_t* sched;                  // {heavy tiles, tiles in the order, heavy lanes per wave, slices, chunk_len} (device_layout.h): the words 32 entries past the cost array (grow_render_buffers)
};

int plan_render(const DsrtContext* ctx, const DsrtRenderDesc* desc, uint8_t* d_rgb8, float* d_f32, const BatchInput* batch, const AccumInput* acc, RenderPlan& p) {
    if (!ctx || !desc || (!d_rgb8 && !acc)) { set_error("dsrt_render: null argument"); return DSRT_ERR_INVALID; }
    const PackedScene* scp = resident_scene(ctx, "dsrt_render");
    if (!scp) return DSRT_ERR_NO_SCENE;
    const PackedScene& sc = *scp;
    if (desc->rng_mode != 0 && desc->rng_mode != 1) { set_error("dsrt_render: rng_mode must be 0 (reference LCG stream per pixel) or 1 (Philox4x32-10 stream per sample)"); return DSRT_ERR_INVALID; }
    if (desc->math_mode != 0 && desc->math_mode != 1) { set_error("dsrt_render: math_mode must be 0 (deterministic sin / cos / pow shared with the CPU oracle) or 1 (the device math library's)"); return DSRT_ERR_INVALID; }
    p.device_libm = desc->math_mode == 1;
    p.rl = &render_launchers(p.device_libm);
    if (desc->tune[3] & ~DSRT_TUNE_FLAG_MASK) { set_error("dsrt_render: tune[3] has bits set that this ABI version does not define (DSRT_TUNE_* in include/dsrt.h)"); return DSRT_ERR_INVALID; }
    const uint32_t flags = (uint32_t)desc->tune[3];
    const uint32_t xp = experiment_word();
    const bool lean = sc.lean && !(xp & (1u << 24));
    Tiling& t = p.t;
    if (!make_tiling(*desc, t)) { set_error("dsrt_render: bad size, tile or shard"); return DSRT_ERR_INVALID; }

    RenderArgs& a = p.a;
    std::memset(&a, 0, sizeof a);
    a.scene = sc.view;
    FrameParams& f = a.frame;
    const FrameState& fs = ctx->frame;
    pack_camera(fs.camera, f.cam);
    f.sun_dir[0] = fs.sun_dir.x; f.sun_dir[1] = fs.sun_dir.y; f.sun_dir[2] = fs.sun_dir.z;
    f.sun_radiance[0] = fs.sun_radiance.x; f.sun_radiance[1] = fs.sun_radiance.y; f.sun_radiance[2] = fs.sun_radiance.z;
    f.sun_enabled = fs.sun_enabled;
    f.width = desc->width; f.height = desc->height;
    f.plan_spp = desc->spp < 1 ? 1 : desc->spp;                         // src/gpu_render.cu:987-988
    f.spp = acc ? acc->count : f.plan_spp;                               // what the launch renders of each pixel: work items, slices and the pre-pass count these
    f.sample_first = acc ? acc->first : 0;
    f.sample_stride = acc ? acc->stride : 1;
    f.max_depth = desc->max_depth > 0 ? desc->max_depth : 12;           // :723-725
    f.inv_gamma = inv_gamma_of(*desc);
    f.seed32 = (uint32_t)(desc->seed & 0xFFFFFFFFu);
    f.seed_hi = (uint32_t)(desc->seed >> 32);
    f.tile = t.tile; f.tiles_x = t.tiles_x; f.tiles_y = t.tiles_y;
    f.shard_rank = desc->shard_rank; f.shard_count = desc->shard_count > 1 ? desc->shard_count : 1;
    f.local_tiles = t.mine;
    if ((unsigned long long)t.mine * (unsigned long long)(t.tile * t.tile) >= (1ull << 31)) { set_error("dsrt_render: image too large (2^31 pixels per shard)"); return DSRT_ERR_INVALID; }
    uint32_t total_items = (uint32_t)t.mine * (uint32_t)(t.tile * t.tile);
    f.compact_output = desc->shard_count > 1 ? 1 : 0;
    p.chunks = 1; p.chunk_len = f.spp;
    f.light_chunk_len = f.spp;
    p.frames = batch ? batch->frames : 1;
    if (batch) {
        if (p.frames < 1 || !batch->cameras || !batch->sun_dirs) { set_error("dsrt_render_batch: no frames"); return DSRT_ERR_INVALID; }
        if (desc->collect_counters || desc->checked) { set_error("dsrt_render_batch uses the production kernel only (no counters, not checked)"); return DSRT_ERR_INVALID; }
        // 32-bit output indices and work-item numbers: frames x pixels (x 8 sample slices in rng_mode 1) stay below 2^32
        const unsigned long long frame_px = desc->shard_count > 1 ? (unsigned long long)t.padded * t.tile * t.tile : (unsigned long long)desc->width * desc->height;
        if ((unsigned long long)p.frames * frame_px * (desc->rng_mode == 1 ? 16ull : 1ull) >= (1ull << 32)) {
            set_error("dsrt_render_batch: too many pixels in one batch (split the sequence)"); return DSRT_ERR_INVALID;
        }
    }
    p.out_pixels = (desc->shard_count > 1 ? (size_t)t.padded * t.tile * t.tile : (size_t)desc->width * desc->height) * (size_t)p.frames;
    p.own_sums = desc->rng_mode == 1 && !acc;
    if (desc->rng_mode == 1) {
        // a pixel's samples are independent streams: pixels of tiles that see geometry are split into 8 work items.  More slices cost
        // more in half-empty advance passes than their shorter tail saves; fewer leave whole waves without work at the end of a small
        // job, which sample stealing (inside a wave, path_machine.h) cannot repair.  One rank's share of an 8-GPU 1080p x 1000 frame,
        // stealing on: 1 / 2 / 4 / 8 / 16 / 32 / 64 slices = 307 / 289 / 188 / 171 / 181 / 191 / 203 ms; whole frame on one GPU
        // 1091 / 1076 / 1063 / 1050 / 1047 (profiles/r02/README.md).  An item's integer sums are 32-bit in units of 2^-20: at most 4095
        // samples per item, so with more samples than that every pixel is sliced, whatever its tile sees.
        int chunk_len = (f.spp + 7) / 8;
        if ((xp >> 8) & 0xFFFu) chunk_len = (f.spp + (int)((xp >> 8) & 0xFFFu) - 1) / (int)((xp >> 8) & 0xFFFu);   // experiment: slices per pixel
        // Sample sets: a set of few samples per pixel (one of many interleaved passes) is not cut below kSetMinItem samples per item.  One of ten passes
        // of the 1080p x 1000 near frame (100 samples): 8 slices of 13 = 114.6 ms, 4 / 2 / 1 slices = 87 / 86 / 88 ms; passes of 250 samples: 189 ms with 8
        // slices, 190-198 with fewer (slices forced by development switch bits 8-19).  dsrt_render keeps its own cut.
        constexpr int kSetMinItem = 32;
        if (acc && !((xp >> 8) & 0xFFFu)) chunk_len = std::max(chunk_len, std::min(f.spp, kSetMinItem));
        if (chunk_len < 1) chunk_len = 1;
        if (chunk_len > 4095) chunk_len = 4095;
        p.chunk_len = chunk_len;
        p.chunks = (f.spp + chunk_len - 1) / chunk_len;
        // Background pixels (tiles that see no geometry) are cut too, but not below kLightLen samples per item: uncut, their 1000-sample
        // items are the longest jobs of a frame and the light queue is served last (one of 8 shares of the near frame 166 -> 149 ms, frame
        // 70 60 -> 43 ms); cut as finely as the heavy pixels, their three 64-bit atomics per item cost the 250-spp sequence, whose frames
        // overlap and have no tail to lose, a fifth of its frame rate (47 -> 38 frames/s).
        {
            const int code = (int)((xp >> 28) & 3u);                                          // experiment
            const int kLightLen = code == 0 ? 128 : (code == 1 ? 64 : (code == 2 ? 256 : 512));
            f.light_chunk_len = (xp & 0x80000000u) ? f.spp : std::max(chunk_len, kLightLen);
            if (f.light_chunk_len > 4095) f.light_chunk_len = 4095;
        }
        if (desc->width > 65535 || desc->height > 65535) { set_error("dsrt_render: rng_mode 1 hands samples between lanes with 16-bit pixel coordinates (width, height <= 65535)"); return DSRT_ERR_INVALID; }
        if ((unsigned long long)total_items * 64ull >= (1ull << 32)) { set_error("dsrt_render: image too large for rng_mode 1 (more than 2^32 sample slices)"); return DSRT_ERR_INVALID; }
        total_items *= 64u;                                     // upper bound (the pre-pass picks 8 to 64 slices per heavy pixel): sizes the grid only
        if (acc) {                                              // the caller's sums, added to (the context's own: grow_render_buffers; 24 bytes per pixel)
            a.accum_fixed = acc->sum;
            a.accum_sq = acc->sum_sq;
        }
    }
    a.out_rgb8 = d_rgb8;
    a.out_f32 = d_f32;
    a.queue = ctx->ctrl.p;
    a.queue_light = ctx->ctrl.p + kQueueLightWord;
    a.flags = ctx->ctrl.p + 1;
    a.counters = (uint64_t*)(ctx->ctrl.p + 4);

    if (desc->stack_entries != 0 && desc->stack_entries != kLdsStackEntries) { set_error("dsrt_render: stack_entries must be 0 or 8"); return DSRT_ERR_INVALID; }
    const int resident_blocks = ctx->num_cus * 4;                         // 4 waves per SIMD = 4 workgroups of 4 waves per CU (render_kernel.hip)
    p.blocks = resident_blocks;                                           // persistent: exactly the resident set
    if ((xp >> 20) & 7u) p.blocks = std::max(1, resident_blocks >> ((xp >> 20) & 7u));     // experiment: a fraction of it (frames that overlap)
    {
        const long long needed = ((long long)total_items + kThreadsPerBlock - 1) / kThreadsPerBlock;
        if (needed < p.blocks && !batch) p.blocks = (int)(needed > 0 ? needed : 1);
    }
    a.spill_entries = sc.view.stack_need > kLdsStackEntries ? sc.view.stack_need - kLdsStackEntries : 0;
    a.spill_stride = (uint32_t)((size_t)p.blocks * kThreadsPerBlock);                  // lanes
    a.min_walk_iters = desc->tune[0] > 0 ? desc->tune[0] : 64;      // (192 when the rays walk the certified second tree: set below, once a.accel is known)
    a.advance_budget = desc->tune[1] > 0 ? desc->tune[1] : 12;
    a.leaf_ratio4 = desc->tune[2] > 0 ? desc->tune[2] : 10;            // (16 until the node loop looked at its votes every other iteration: profiles/r03/ab_loop_knobs_after_unroll.jsonl)
    a.deal_leaves = (xp & 128u) ? 0 : 1;
    // The certified second tree (pack_scene): used when it is resident, the host has not asked for the plain reference walk, and every camera of the launch is within
    // 30 scene extents of the scene's centre (the widening of the second tree's boxes covers the rounding of (box - origin) up to there; bounce and shadow rays start
    // on the geometry).  Otherwise every ray walks the reference tree, as without the option.
    a.accel = 0;
    if (sc.has_second_tree && !(flags & DSRT_TUNE_REFERENCE_WALK)) {
        auto near_enough = [&](const DsrtF3& o) {
            const double dx = (double)o.x - sc.scene_centre[0], dy = (double)o.y - sc.scene_centre[1], dz = (double)o.z - sc.scene_centre[2];
            return std::sqrt(dx * dx + dy * dy + dz * dz) <= 30.0 * (double)sc.scene_extent;
        };
        bool ok = true;
        if (batch) { for (int i = 0; i < batch->frames && ok; ++i) ok = near_enough(batch->cameras[i].origin); }
        else ok = near_enough(fs.camera.origin);
        a.accel = ok ? 1 : 0;
    }
    a.audit = a.accel && desc->collect_counters == 3 ? 1 : 0;
    // Walks of the second tree are a third shorter, so an advance pass is dearer against a node iteration than on the reference tree: the traverse phase stays three times
    // longer before it yields (interleaved medians, near frame: 760 -> 741 ms in rng_mode 0, 734 -> 701 in rng_mode 1; the reference walk gains nothing from it).
    if (a.accel && desc->tune[0] <= 0) a.min_walk_iters = 192;
    // ... and its leaves come sooner: the node loop yields to the leaf pass at 0.6 parked lane-slots per descending lane instead of 1.0 (rng_mode 0: near frame -0.5 ... -1.1 %,
    // frame 85 -5 %, frame 92 -2 %, one of 8 shares -1.6 %, far frames unchanged; rng_mode 1 loses 1 % and keeps 1.0: profiles/r04/ab_leaf_ratio_*.jsonl).
    if (a.accel && desc->rng_mode == 0 && desc->tune[2] <= 0) a.leaf_ratio4 = 6;
    a.helpers = (flags & DSRT_TUNE_NO_HELPERS) ? 0 : 1;
    a.steal = ((flags & DSRT_TUNE_NO_STEALING) ? 0 : 1) | (((xp & (1u << 27)) && desc->collect_counters) ? 8 : 0);      // (8: timing image, counting build)
    // rng_mode 0: waves that hold a pixel of a heavy tile get issue priority over waves that only hold background pixels (render_body).
    // Interleaved medians, 1080p x 1000: near frame 1117 -> 1108 ms, frame 95 801 -> 785 ms.  Finer grades (the top quarter and sixteenth of
    // the order above the rest) were tried in round 2 and moved nothing consistently (profiles/r02/ab_issue_priority.jsonl); they are gone.
    a.hot = (flags & DSRT_TUNE_NO_PRIORITY) ? 0 : 1;

    // Pre-pass for this camera: costliest-first tile order (scheduling only) and removal of tiles that are provably empty (exact:
    // see dsrt_tile_cost_kernel).  DSRT_TUNE_NATURAL_ORDER switches both off, DSRT_TUNE_NO_CULLING keeps the order but culls nothing; counting builds never
    // cull, so that their counters cover every sample.  The words 32 and 33 entries past the cost array receive the number of
    // heavy tiles and the number of tiles in the order.
    p.pre_stride = (size_t)t.mine + 64;
    if (p.pre_stride * (size_t)p.frames >= ((size_t)1 << 32)) { set_error("dsrt_render_batch: too many tiles in one batch (split the sequence)"); return DSRT_ERR_INVALID; }
    p.pre = batch ? PrePass::Batch : ((flags & 3u) != DSRT_TUNE_NATURAL_ORDER && t.mine > 0 ? PrePass::Ordered : PrePass::Natural);
    p.cull = batch ? (flags & 3u) == 0u : (flags & 3u) != DSRT_TUNE_NO_CULLING && desc->collect_counters == 0;
    // The probe (probe_tiles) is worth its 0.5 % only when a pixel is a long chain; DSRT_TUNE_NO_PROBE switches it off.
    // Only with the reference's stream: in rng_mode 1 a pixel is cut into slices and lanes share samples, so there is no long chain to start
    // early, and the coverage order alone is better (interleaved medians, near frame: 1046 -> 1037 ms, one of 8 shares 176 -> 167 ms).
    p.probe = p.pre != PrePass::Natural && !(flags & DSRT_TUNE_NO_PROBE) && desc->rng_mode == 0 && f.spp >= 64 * kProbeSpp;
    p.probe_spp = (!batch && (xp & 64u)) ? 2 * kProbeSpp : kProbeSpp;                  // experiment (a batch's probes ignore it)

    const bool count = desc->collect_counters != 0;
    RenderVariant& v = p.variant;
    v = RenderVariant{};
    v.rng_mode = desc->rng_mode;
    v.count = count; v.checked = count || desc->checked != 0; v.anyhit = desc->collect_counters != 2;
    v.lean = lean; v.sets = acc != nullptr; v.moments = acc && acc->sum_sq; v.listed = acc && acc->mask;
    return DSRT_OK;
}

// Each buffer by its own size: a failed allocation leaves no stale sibling.
int grow_render_buffers(DsrtContext* ctx, RenderPlan& p) {
    RenderArgs& a = p.a;
    int rc;
    if (p.own_sums) {
        if ((rc = ctx->accum_fixed.grow(p.out_pixels * 3))) return rc;
        a.accum_fixed = ctx->accum_fixed.p;
    }
    if (a.spill_entries > 0 && (rc = ctx->spill.grow((size_t)a.spill_stride * (size_t)a.spill_entries))) return rc;
    a.spill = ctx->spill.p;
    if ((rc = ctx->tile_cost.grow(p.pre_stride * (size_t)p.frames)) || (rc = ctx->tile_order.grow(p.pre_stride * (size_t)p.frames)) ||
        (rc = ctx->tile_work.grow(p.pre_stride)) || (rc = ctx->tile_tmp.grow(p.pre_stride))) return rc;
    if (p.pre == PrePass::Batch && (rc = ctx->batch_table.grow(2 * (size_t)p.frames))) return rc;
    if (p.probe && (rc = ctx->probe_queue.grow(1024))) return rc;
    if (p.variant.listed) {
        const size_t tile_pixels = (size_t)p.t.mine * (size_t)(p.t.tile * p.t.tile);     // the two lists, and a word per 8x8 block behind them (launch_pixel_list)
        if ((rc = ctx->pixel_list.grow(tile_pixels + tile_pixels / 64))) return rc;
        a.list = ctx->pixel_list.p;
    }
    p.sched = ctx->tile_cost.p + p.t.mine + 32;
    a.sched = p.sched;
    if (p.variant.listed) a.list_len = p.sched + kListLenSched;
    return DSRT_OK;
}

// Probe: the render kernel itself at a few samples per pixel (reference stream, nothing stored) measures what every tile of the frame `pa` describes
// costs; the heavy tiles of its order (`at` entries into the context's order and sched arrays) are then re-sorted by that.
// Its work items are tiny, so the probe has 64 queue words of its own (path_machine.h, ST_FETCH): on the frame's single queue word
// the same launch took 27 ms.  It leaves the frame's queue words used: the caller zeroes `ctrl` behind its last probe, and, where probes follow each
// other, before each (zero_ctrl_first).
int probe_tiles(DsrtContext* ctx, const RenderPlan& p, RenderArgs pa, size_t at, bool zero_ctrl_first, hipStream_t stream) {
    pa.frame.spp = p.probe_spp;
    pa.out_f32 = nullptr; pa.accum_fixed = nullptr; pa.counters = nullptr;
    pa.sched = p.sched + at;
    pa.frame.tile_order = ctx->tile_order.p + at;
    pa.tile_work = ctx->tile_work.p;
    pa.probe_queue = ctx->probe_queue.p;
    HIP_TRY(hipMemsetAsync(ctx->probe_queue.p, 0, 1024 * sizeof(uint32_t), stream));
    HIP_TRY(hipMemsetAsync(ctx->tile_work.p, 0, (size_t)p.t.mine * sizeof(uint32_t), stream));
    if (zero_ctrl_first) HIP_TRY(hipMemsetAsync(ctx->ctrl.p, 0, kCtrlWords * sizeof(uint32_t), stream));
    HIP_TRY(p.rl->launch_probe(pa, p.blocks, p.variant.lean, stream));
    HIP_TRY(launch_tile_reorder(ctx->tile_work.p, ctx->tile_order.p + at, ctx->tile_tmp.p, p.sched + at, stream));
    return DSRT_OK;
}

// Batch: every frame's pre-pass (exact culling + coverage order), its results left pre_stride apart; then one small kernel turns the counts into the
// table the render kernel looks work items up in.  Slices stay at the host's 8 (resident_lanes = 0: the pool is never short of heavy pixels).
int prepass_batch(DsrtContext* ctx, RenderPlan& p, const BatchInput& batch, hipStream_t stream) {
    RenderArgs& a = p.a;
    const size_t frames = (size_t)p.frames;
    HIP_TRY(hipMemsetAsync(a.out_rgb8, 0, p.out_pixels * 3, stream));                          // culled pixels are never written
    if (a.out_f32) HIP_TRY(hipMemsetAsync(a.out_f32, 0, p.out_pixels * 3 * sizeof(float), stream));
    ctx->batch_host.assign(2 * frames, BatchFrame{});
    for (size_t i = 0; i < frames; ++i) {
        BatchFrame& e = ctx->batch_host[i];
        pack_camera(batch.cameras[i], e.cam);
        e.sun_dir[0] = batch.sun_dirs[i].x; e.sun_dir[1] = batch.sun_dirs[i].y; e.sun_dir[2] = batch.sun_dirs[i].z;
        e.order_base = (uint32_t)(p.pre_stride * i);
        e.image_slot = (uint32_t)i;
        ctx->batch_host[frames + i] = e;                                                  // the frame's second entry (device_layout.h, BatchFrame)
    }
    HIP_TRY(hipMemcpyAsync(ctx->batch_table.p, ctx->batch_host.data(), 2 * frames * sizeof(BatchFrame), hipMemcpyHostToDevice, stream));
    HIP_TRY(launch_tile_order(a.scene, a.frame, ctx->tile_cost.p, ctx->tile_order.p, p.sched, (uint32_t)p.chunks, 0u, p.cull, stream,
                              ctx->batch_table.p, (uint32_t)frames, (uint32_t)p.pre_stride));
    // rng_mode 0 at enough samples for a pixel to be a long chain: every frame's heavy tiles re-sorted by measured cost, as for a single
    // frame -- one probe per frame, 6 ms each at 1080p, against a frame of a second
    if (p.probe) {
        for (size_t i = 0; i < frames; ++i) {
            RenderArgs pa = a;
            std::memcpy(pa.frame.cam, ctx->batch_host[i].cam, sizeof pa.frame.cam);
            std::memcpy(pa.frame.sun_dir, ctx->batch_host[i].sun_dir, 3 * sizeof(float));
            if (int rc = probe_tiles(ctx, p, pa, p.pre_stride * i, true, stream)) return rc;
        }
        HIP_TRY(hipMemsetAsync(ctx->ctrl.p, 0, kCtrlWords * sizeof(uint32_t), stream));
    }
    HIP_TRY(launch_batch_table(ctx->batch_table.p, p.sched, (uint32_t)p.pre_stride, (uint32_t)frames, (uint32_t)(p.t.tile * p.t.tile), p.variant.rng_mode, a.frame.spp,
                               a.frame.light_chunk_len, ctx->ctrl.p + 2, stream));
    a.batch = ctx->batch_table.p; a.batch_order = ctx->tile_order.p; a.batch_frames = 2u * (uint32_t)frames;
    a.batch_frame_pixels = (uint32_t)(p.out_pixels / frames);        // whole images, or the padded compact shard buffers, one after another
    return DSRT_OK;
}

// One frame, costliest tiles first.
int prepass_ordered(DsrtContext* ctx, RenderPlan& p, hipStream_t stream) {
    RenderArgs& a = p.a;
    if (p.cull && a.out_rgb8) {                                 // culled pixels are never written: they are the zeros put here (an accumulate launch adds nothing for them)
        HIP_TRY(hipMemsetAsync(a.out_rgb8, 0, p.out_pixels * 3, stream));
        if (a.out_f32) HIP_TRY(hipMemsetAsync(a.out_f32, 0, p.out_pixels * 3 * sizeof(float), stream));
    }
    HIP_TRY(launch_tile_order(a.scene, a.frame, ctx->tile_cost.p, ctx->tile_order.p, p.sched, (uint32_t)p.chunks,
                              (uint32_t)p.blocks * (uint32_t)kThreadsPerBlock, p.cull, stream));
    a.frame.tile_order = ctx->tile_order.p;
    if (p.probe) {
        if (int rc = probe_tiles(ctx, p, a, 0, false, stream)) return rc;
        HIP_TRY(hipMemsetAsync(ctx->ctrl.p, 0, kCtrlWords * sizeof(uint32_t), stream));
    }
    return DSRT_OK;
}

// One frame, every tile in the heavy queue, natural order.
int prepass_natural(const RenderPlan& p, hipStream_t stream) {
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)p.sched, p.t.mine, 2, stream));
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)(p.sched + 2), 64, 1, stream));
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)(p.sched + 3), p.chunks, 1, stream));
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)(p.sched + 4), p.chunk_len, 1, stream));
    return DSRT_OK;
}

int launch_and_resolve(const RenderPlan& p, hipStream_t stream) {
    const RenderArgs& a = p.a;
    if (p.pre == PrePass::Batch) HIP_TRY(p.rl->launch_render_batch(a, p.variant.rng_mode, p.blocks, p.variant.lean, stream));
    else HIP_TRY(p.rl->launch_render(a, p.variant, p.blocks, stream));
    if (p.own_sums) HIP_TRY(launch_resolve(a.accum_fixed, a.frame.spp, a.frame.inv_gamma, p.device_libm, p.out_pixels, a.out_rgb8, a.out_f32, nullptr, nullptr, stream));
    return DSRT_OK;
}

// The counters of a finished launch (launch_finish has waited for it), as DsrtStats.
int read_render_stats(DsrtContext* ctx, const RenderPlan& p, DsrtStats* stats) {
    uint32_t ctrl[kCtrlWords];
    HIP_TRY(hipMemcpy(ctrl, ctx->ctrl.p, sizeof ctrl, hipMemcpyDeviceToHost));
    stats->device_flags = ctrl[1];
    stats->waves_launched = p.blocks * kWavesPerBlock;
    stats->lds_stack_entries = kLdsStackEntries;
    uint64_t cnt[kNumCounters];
    std::memcpy(cnt, &ctrl[4], sizeof cnt);
    stats->samples = cnt[C_SAMPLES]; stats->rays = cnt[C_RAYS]; stats->primary_hits = cnt[C_PRIMARY_HITS];
    stats->box_fetches = cnt[C_BOX_FETCHES]; stats->nodes_entered = cnt[C_NODES_ENTERED]; stats->internal_entered = cnt[C_INTERNAL_ENTERED];
    stats->tri_tests = cnt[C_TRI_TESTS]; stats->hit_updates = cnt[C_HIT_UPDATES]; stats->sphere_tests = cnt[C_SPHERE_TESTS];
    stats->shaded_hits = cnt[C_SHADED_HITS]; stats->tex_fetches = cnt[C_TEX_FETCHES]; stats->stack_spills = cnt[C_STACK_SPILLS];
    stats->max_stack = cnt[C_MAX_STACK];
    stats->node_slots = cnt[C_NODE_SLOTS]; stats->tri_slots = cnt[C_TRI_SLOTS]; stats->adv_slots = cnt[C_ADV_SLOTS]; stats->adv_active = cnt[C_ADV_ACTIVE];
    stats->idle_at_leaf = cnt[C_IDLE_AT_LEAF]; stats->idle_waiting = cnt[C_IDLE_WAITING]; stats->idle_done = cnt[C_IDLE_DONE];
    stats->wave_ticks = cnt[C_WAVE_TICKS];
    stats->certificate_fallbacks = cnt[C_CERT_FALLBACKS];
    stats->certificate_audited = cnt[C_AUDITED]; stats->certificate_audit_mismatches = cnt[C_AUDIT_MISMATCHES];
    stats->certified_tree_used = p.a.accel;
    {   // time marks relative to the first wave's start, in ms (0 when the mark was never passed)
        const double t0 = (double)~cnt[C_T_FIRST];
        stats->heavy_queue_empty_ms = cnt[C_T_HEAVY_EMPTY] ? (float)(((double)~cnt[C_T_HEAVY_EMPTY] - t0) * 1e-5) : 0.0f;
        stats->light_queue_empty_ms = cnt[C_T_LIGHT_EMPTY] ? (float)(((double)~cnt[C_T_LIGHT_EMPTY] - t0) * 1e-5) : 0.0f;
        stats->last_wave_exit_ms = cnt[C_T_LAST] ? (float)(((double)cnt[C_T_LAST] - t0) * 1e-5) : 0.0f;
    }
    stats->visits_depth_lt6 = cnt[C_VISITS_LT6]; stats->visits_depth_lt9 = cnt[C_VISITS_LT9]; stats->visits_depth_lt12 = cnt[C_VISITS_LT12];
    uint32_t live = 0;
    HIP_TRY(hipMemcpy(&live, p.sched + 1, sizeof live, hipMemcpyDeviceToHost));
    stats->tiles_total = (uint64_t)p.t.mine; stats->tiles_culled = (uint64_t)p.t.mine - live;
    return DSRT_OK;
}

}  // namespace

int dsrt::render_impl(DsrtContext* ctx, const DsrtRenderDesc* desc, uint8_t* d_rgb8, float* d_f32, void* stream_v, DsrtStats* stats, const BatchInput* batch,
                      const AccumInput* acc) {
    RenderPlan p;
    int rc = plan_render(ctx, desc, d_rgb8, d_f32, batch, acc, p);          // every refusal: nothing has been enqueued
    if (rc) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t stream = (hipStream_t)stream_v;
    if ((rc = grow_render_buffers(ctx, p))) return rc;
    // a context's working buffers serve one render at a time; its own sums (24 bytes per pixel) and its queue, flag and counter words start at zero
    if ((rc = launch_begin(ctx, stream, {{p.own_sums ? p.a.accum_fixed : nullptr, p.out_pixels * 3 * sizeof(unsigned long long)}, {ctx->ctrl.p, kCtrlWords * sizeof(uint32_t)}}))) return rc;
    switch (p.pre) {
        case PrePass::Batch: rc = prepass_batch(ctx, p, *batch, stream); break;
        case PrePass::Ordered: rc = prepass_ordered(ctx, p, stream); break;
        case PrePass::Natural: rc = prepass_natural(p, stream); break;
    }
    // a masked launch: the lists of active pixels, from the mask and the order the pre-pass has just left (and the sample counts of those pixels)
    if (!rc && p.variant.listed)
        HIP_TRY(launch_pixel_list(p.a.frame, p.a.frame.tile_order, p.sched, acc->mask, ctx->pixel_list.p, p.sched + kListLenSched, acc->n, (uint32_t)acc->count, stream));
    if (rc || (rc = launch_clock(ctx, stream, stats)) || (rc = launch_and_resolve(p, stream)) || (rc = launch_finish(ctx, stream, stats)) || !stats) return rc;
    if ((rc = read_render_stats(ctx, p, stats))) return rc;
    return flags_result("render", stats->device_flags);
}

extern "C" {

int dsrt_shard_layout(const DsrtRenderDesc* desc, int* tiles_total, int* tiles_this_shard, int* tiles_per_shard_padded, size_t* rgb8_bytes_padded) {
    Tiling t;
    if (!desc || !make_tiling(*desc, t)) { set_error("dsrt_shard_layout: bad descriptor"); return DSRT_ERR_INVALID; }
    if (tiles_total) *tiles_total = t.total;
    if (tiles_this_shard) *tiles_this_shard = t.mine;
    if (tiles_per_shard_padded) *tiles_per_shard_padded = t.padded;
    if (rgb8_bytes_padded) *rgb8_bytes_padded = (size_t)t.padded * t.tile * t.tile * 3;
    return DSRT_OK;
}

int dsrt_render(DsrtContext* ctx, const DsrtRenderDesc* desc, uint8_t* d_rgb8, float* d_f32, void* stream, DsrtStats* stats) {
    return render_impl(ctx, desc, d_rgb8, d_f32, stream, stats, nullptr);
}

int dsrt_render_batch(DsrtContext* ctx, const DsrtRenderDesc* desc, int frames, const GPUCamera* cameras, const float* sun_dirs_xyz, uint8_t* d_rgb8, float* d_f32,
                      void* stream, DsrtStats* stats) {
    return dsrt::guarded("dsrt_render_batch", [&]() -> int {
        if (frames < 1 || !cameras || !sun_dirs_xyz) { set_error("dsrt_render_batch: null argument"); return DSRT_ERR_INVALID; }
        std::vector<DsrtF3> suns((size_t)frames);
        for (int i = 0; i < frames; ++i) suns[(size_t)i] = DsrtF3{sun_dirs_xyz[3 * i], sun_dirs_xyz[3 * i + 1], sun_dirs_xyz[3 * i + 2]};
        const BatchInput b{frames, cameras, suns.data()};
        return render_impl(ctx, desc, d_rgb8, d_f32, stream, stats, &b);
    });
}

int dsrt_deinterleave_batch(DsrtContext* ctx, const DsrtRenderDesc* desc, int frames, const uint8_t* d_gathered, uint8_t* d_rgb8_images, void* stream) {
    Tiling t;
    if (!ctx || !desc || frames < 1 || !d_gathered || !d_rgb8_images || !make_tiling(*desc, t)) { set_error("dsrt_deinterleave_batch: bad argument"); return DSRT_ERR_INVALID; }
    HIP_TRY(hipSetDevice(ctx->device));
    const int count = desc->shard_count > 1 ? desc->shard_count : 1;
    const size_t part = (size_t)t.padded * t.tile * t.tile * 3, image = (size_t)desc->width * desc->height * 3;
    // the gather of sharded batch launches: rank r's buffer holds its part of frame 0, of frame 1, ...; rank r + 1's follows `frames` parts on
    for (int f = 0; f < frames; ++f)
        HIP_TRY(launch_deinterleave(d_gathered + (size_t)f * part, d_rgb8_images + (size_t)f * image, desc->width, desc->height, t.tile, t.tiles_x, count,
                                    part * (size_t)frames, (hipStream_t)stream));
    return DSRT_OK;
}

int dsrt_deinterleave_tiles(DsrtContext* ctx, const DsrtRenderDesc* desc, const uint8_t* d_gathered, uint8_t* d_rgb8_image, void* stream) {
    Tiling t;
    if (!ctx || !desc || !d_gathered || !d_rgb8_image || !make_tiling(*desc, t)) { set_error("dsrt_deinterleave_tiles: bad argument"); return DSRT_ERR_INVALID; }
    HIP_TRY(hipSetDevice(ctx->device));
    const int count = desc->shard_count > 1 ? desc->shard_count : 1;
    HIP_TRY(launch_deinterleave(d_gathered, d_rgb8_image, desc->width, desc->height, t.tile, t.tiles_x, count, (size_t)t.padded * t.tile * t.tile * 3,
                                (hipStream_t)stream));
    return DSRT_OK;
}

int dsrt_render_batch_to_host(DsrtContext* ctx, const DsrtRenderDesc* desc, int frames, const GPUCamera* cameras, const float* sun_dirs_xyz, uint8_t* h_rgb8,
                              DsrtStats* stats) {
    return dsrt::guarded("dsrt_render_batch_to_host", [&]() -> int {
    if (!ctx || !desc || !h_rgb8 || frames < 1) { set_error("dsrt_render_batch_to_host: null argument"); return DSRT_ERR_INVALID; }
    HIP_TRY(hipSetDevice(ctx->device));
    const Staged s[1] = {{h_rgb8, (size_t)desc->width * desc->height * 3 * (size_t)frames, Dir::Out}};
    DsrtStats local;
    return staged_call(s, [&](void* const* d) { return dsrt_render_batch(ctx, desc, frames, cameras, sun_dirs_xyz, (uint8_t*)d[0], nullptr, nullptr, stats ? stats : &local); });
    });
}

int dsrt_render_to_host(DsrtContext* ctx, const DsrtRenderDesc* desc, uint8_t* h_rgb8, float* h_f32, DsrtStats* stats) {
    return dsrt::guarded("dsrt_render_to_host", [&]() -> int {
    if (!ctx || !desc || !h_rgb8) { set_error("dsrt_render_to_host: null argument"); return DSRT_ERR_INVALID; }
    if (desc->shard_count > 1) { set_error("dsrt_render_to_host renders whole images only"); return DSRT_ERR_INVALID; }
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t px = (size_t)desc->width * desc->height;
    const Staged s[2] = {{h_rgb8, px * 3, Dir::Out}, {h_f32, px * 3 * sizeof(float), Dir::Out}};
    DsrtStats local;
    return staged_call(s, [&](void* const* d) { return dsrt_render(ctx, desc, (uint8_t*)d[0], (float*)d[1], nullptr, stats ? stats : &local); });
    });
}

}  // extern "C"
