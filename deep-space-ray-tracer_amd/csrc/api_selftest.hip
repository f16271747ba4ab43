// api_selftest.hip -- the self-test hooks of include/dsrt.h: poke and read the resident scene's words, and run the device math, the kernel helpers and the
// Philox stream on plain arrays; read what the scheduling pre-pass of the context's last launch left, and run its three array kernels on plain arrays.
// Calls the self-test launchers of selftest_kernel.hip and schedule_kernel.hip; nothing calls into this file.
#include "api_internal.h"

using namespace dsrt;

extern "C" {

int dsrt_selftest_poke_node_word(DsrtContext* ctx, size_t word_index, uint32_t value, uint32_t* old_value) {
    if (!resident_scene(ctx, "dsrt_selftest_poke_node_word")) return DSRT_ERR_NO_SCENE;
    if (word_index >= ctx->scene->pairs.n * 4) { set_error("dsrt_selftest_poke_node_word: word index beyond the node records"); return DSRT_ERR_INVALID; }
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipDeviceSynchronize());
    uint32_t* w = reinterpret_cast<uint32_t*>(ctx->scene->pairs.p) + word_index;
    if (old_value) HIP_TRY(hipMemcpy(old_value, w, 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(w, &value, 4, hipMemcpyHostToDevice));
    return DSRT_OK;
}

int dsrt_selftest_read_scene_words(DsrtContext* ctx, int array, size_t first_word, size_t n_words, uint32_t* out) {
    if (!resident_scene(ctx, "dsrt_selftest_read_scene_words")) return DSRT_ERR_NO_SCENE;
    const PackedScene& sc = *ctx->scene;
    if (array < 0 || array > 2) { set_error("dsrt_selftest_read_scene_words: no such array"); return DSRT_ERR_INVALID; }
    const DevBuf<float4>& buf = array == 0 ? sc.pairs : array == 1 ? sc.tri_pairs : sc.tri_shade;
    const size_t words = buf.n * 4;
    if (first_word > words || n_words > words - first_word) { set_error("dsrt_selftest_read_scene_words: range beyond the array"); return DSRT_ERR_INVALID; }
    if (!out || !n_words) return DSRT_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, reinterpret_cast<const uint32_t*>(buf.p) + first_word, n_words * 4, hipMemcpyDeviceToHost));
    return DSRT_OK;
}

int dsrt_selftest_math(DsrtContext* ctx, int fn, const float* x, float y, float* out, int n) {
    if (!ctx || !x || !out || n <= 0 || fn < 0 || fn > 2) { set_error("dsrt_selftest_math: bad argument"); return DSRT_ERR_INVALID; }
    HIP_TRY(hipSetDevice(ctx->device));
    DevBuf<float> dx, dy;
    int rc;
    if ((rc = dx.alloc((size_t)n)) || (rc = dy.alloc((size_t)n))) return rc;
    HIP_TRY(hipMemcpy(dx.p, x, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(launch_math(fn, dx.p, y, dy.p, n, nullptr));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, dy.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return DSRT_OK;
}

int dsrt_selftest_devkat(DsrtContext* ctx, int fn, const float* in12, float* out12, int n) {
    if (!ctx || !in12 || !out12 || n <= 0 || fn < 0 || fn > 5) { set_error("dsrt_selftest_devkat: bad argument"); return DSRT_ERR_INVALID; }
    HIP_TRY(hipSetDevice(ctx->device));
    DevBuf<float> di, dout;
    int rc;
    if ((rc = di.alloc((size_t)n * 12)) || (rc = dout.alloc((size_t)n * 12))) return rc;
    HIP_TRY(hipMemcpy(di.p, in12, (size_t)n * 12 * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(dout.p, 0, (size_t)n * 12 * sizeof(float)));
    HIP_TRY(launch_devkat(fn, di.p, dout.p, n, nullptr));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out12, dout.p, (size_t)n * 12 * sizeof(float), hipMemcpyDeviceToHost));
    return DSRT_OK;
}

int dsrt_selftest_philox(DsrtContext* ctx, uint64_t seed, uint64_t subsequence, int n, uint32_t* ours, uint32_t* rocrand_words) {
    if (!ctx || !ours || !rocrand_words || n <= 0) { set_error("dsrt_selftest_philox: bad argument"); return DSRT_ERR_INVALID; }
    HIP_TRY(hipSetDevice(ctx->device));
    DevBuf<uint32_t> a, b;
    int rc;
    if ((rc = a.alloc((size_t)n)) || (rc = b.alloc((size_t)n))) return rc;
    HIP_TRY(launch_philox(seed, subsequence, n, a.p, b.p, nullptr));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(ours, a.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(rocrand_words, b.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return DSRT_OK;
}

// ---- the scheduling pre-pass (include/dsrt.h, SELFTEST: the scheduling pre-pass) ----

int dsrt_selftest_read_schedule(DsrtContext* ctx, int array, size_t first_word, size_t n_words, uint32_t* out) {
    if (!ctx || !out) { set_error("dsrt_selftest_read_schedule: null argument"); return DSRT_ERR_INVALID; }
    if (array < 0 || array > 4) { set_error("dsrt_selftest_read_schedule: no such array"); return DSRT_ERR_INVALID; }
    const uint32_t* p = nullptr;
    size_t words = 0;
    switch (array) {
        case 0: p = ctx->tile_cost.p; words = ctx->tile_cost.n; break;
        case 1: p = ctx->tile_order.p; words = ctx->tile_order.n; break;
        case 2: p = ctx->tile_work.p; words = ctx->tile_work.n; break;
        case 3: p = reinterpret_cast<const uint32_t*>(ctx->batch_table.p); words = ctx->batch_table.n * (sizeof(BatchFrame) / sizeof(uint32_t)); break;
        default: p = ctx->pixel_list.p; words = ctx->pixel_list.n; break;
    }
    if (!p) { set_error("dsrt_selftest_read_schedule: no launch on this context has used that array yet"); return DSRT_ERR_INVALID; }
    if (!n_words || first_word > words || n_words > words - first_word) { set_error("dsrt_selftest_read_schedule: range beyond the array"); return DSRT_ERR_INVALID; }
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, p + first_word, n_words * 4, hipMemcpyDeviceToHost));
    return DSRT_OK;
}

int dsrt_selftest_tile_order(DsrtContext* ctx, const uint32_t* cost, int n, int tile, uint32_t items_per_pixel, uint32_t resident_lanes, int spp, uint32_t* order,
                             uint32_t* sched5) {
    // (cost and order may be null only when n is 0; a cost word's low bits are a pixel count of the tile: beyond tile^2 the kernel's `* 64` would wrap)
    if (!ctx || !sched5 || n < 0 || (n > 0 && (!cost || !order)) || tile < 8 || tile > 1024 || tile % 8 != 0 || items_per_pixel < 1 || spp < 1) {
        set_error("dsrt_selftest_tile_order: bad argument"); return DSRT_ERR_INVALID;
    }
    for (int t = 0; t < n; ++t)
        if ((cost[t] & 0x7FFFFFFFu) > (uint32_t)(tile * tile)) { set_error("dsrt_selftest_tile_order: a cost word counts more pixels than a tile has"); return DSRT_ERR_INVALID; }
    HIP_TRY(hipSetDevice(ctx->device));
    DevBuf<uint32_t> dc, dord, ds;
    int rc;
    if ((rc = dc.alloc((size_t)n + 1)) || (rc = dord.alloc((size_t)n + 1)) || (rc = ds.alloc(5))) return rc;
    if (n) HIP_TRY(hipMemcpy(dc.p, cost, (size_t)n * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(dord.p, 0xFF, ((size_t)n + 1) * 4));                  // what the kernel does not write stays 0xFFFFFFFF
    HIP_TRY(hipMemset(ds.p, 0xFF, 5 * 4));
    HIP_TRY(launch_tile_order_arrays(dc.p, dord.p, n, tile, ds.p, items_per_pixel, resident_lanes, spp, nullptr));
    HIP_TRY(hipDeviceSynchronize());
    if (n) HIP_TRY(hipMemcpy(order, dord.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(sched5, ds.p, 5 * 4, hipMemcpyDeviceToHost));
    return DSRT_OK;
}

int dsrt_selftest_tile_reorder(DsrtContext* ctx, const uint32_t* work, int n_work, uint32_t* order, int n_order, const uint32_t* sched5) {
    if (!ctx || !sched5 || n_work < 0 || n_order < 0 || (n_work > 0 && !work) || (n_order > 0 && !order) || sched5[0] > (uint32_t)n_order) {
        set_error("dsrt_selftest_tile_reorder: bad argument"); return DSRT_ERR_INVALID;
    }
    for (uint32_t i = 0; i < sched5[0]; ++i)                                   // the kernel reads work[order[i]] of the heavy part
        if (order[i] >= (uint32_t)n_work) { set_error("dsrt_selftest_tile_reorder: an order entry beyond the work array"); return DSRT_ERR_INVALID; }
    HIP_TRY(hipSetDevice(ctx->device));
    DevBuf<uint32_t> dw, dord, dtmp, ds;
    int rc;
    if ((rc = dw.alloc((size_t)n_work + 1)) || (rc = dord.alloc((size_t)n_order + 1)) || (rc = dtmp.alloc((size_t)n_order + 1)) || (rc = ds.alloc(5))) return rc;
    if (n_work) HIP_TRY(hipMemcpy(dw.p, work, (size_t)n_work * 4, hipMemcpyHostToDevice));
    if (n_order) HIP_TRY(hipMemcpy(dord.p, order, (size_t)n_order * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(ds.p, sched5, 5 * 4, hipMemcpyHostToDevice));
    HIP_TRY(launch_tile_reorder(dw.p, dord.p, dtmp.p, ds.p, nullptr));
    HIP_TRY(hipDeviceSynchronize());
    if (n_order) HIP_TRY(hipMemcpy(order, dord.p, (size_t)n_order * 4, hipMemcpyDeviceToHost));
    return DSRT_OK;
}

int dsrt_selftest_batch_table(DsrtContext* ctx, const uint32_t* sched, uint32_t sched_stride, uint32_t frames, uint32_t tt, int rng_mode, int spp, int light_chunk_len,
                              const uint32_t* order_base, uint32_t* table_words, uint32_t* total_items) {
    if (!ctx || !sched || !order_base || !table_words || !total_items || sched_stride < 5 || frames < 1 || frames > 65536 || (rng_mode != 0 && rng_mode != 1) || spp < 1 ||
        light_chunk_len < 1) {
        set_error("dsrt_selftest_batch_table: bad argument"); return DSRT_ERR_INVALID;
    }
    for (uint32_t f = 0; f < frames; ++f)                                      // (n_live - n_heavy is formed unsigned)
        if (sched[(size_t)f * sched_stride] > sched[(size_t)f * sched_stride + 1]) { set_error("dsrt_selftest_batch_table: more heavy tiles than live ones"); return DSRT_ERR_INVALID; }
    HIP_TRY(hipSetDevice(ctx->device));
    // the table as prepass_batch uploads it: both entries of a frame carry its order_base and image slot, the counts are the kernel's to fill
    std::vector<BatchFrame> host(2 * (size_t)frames, BatchFrame{});
    for (uint32_t f = 0; f < frames; ++f) {
        host[f].order_base = order_base[f]; host[f].image_slot = f;
        host[frames + f] = host[f];
    }
    DevBuf<BatchFrame> dt;
    DevBuf<uint32_t> ds, dtotal;
    int rc;
    if ((rc = dt.upload(host)) || (rc = ds.alloc((size_t)frames * sched_stride)) || (rc = dtotal.alloc(1))) return rc;
    HIP_TRY(hipMemcpy(ds.p, sched, (size_t)frames * sched_stride * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(dtotal.p, 0xFF, 4));
    HIP_TRY(launch_batch_table(dt.p, ds.p, sched_stride, frames, tt, rng_mode, spp, light_chunk_len, dtotal.p, nullptr));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(table_words, dt.p, host.size() * sizeof(BatchFrame), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(total_items, dtotal.p, 4, hipMemcpyDeviceToHost));
    return DSRT_OK;
}

}  // extern "C"
