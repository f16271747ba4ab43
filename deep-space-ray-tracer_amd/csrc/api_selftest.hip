// api_selftest.hip -- the self-test hooks of include/dsrt.h: poke and read the resident scene's words, and run the device math, the kernel helpers and the
// Philox stream on plain arrays.  Calls the self-test launchers of render_kernel.hip; nothing calls into this file.
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

}  // extern "C"
