/*
 * oracle_sample_sets.c -- TEST INFRASTRUCTURE, CPU only: the sample sets of include/dsrt.h (dsrt_render_accumulate / dsrt_resolve_accumulated) restated on the
 * CPU on top of the oracle's own rng_mode 1 path (oracle/dsrt_oracle.c: its Philox Rng, camera_ray and ray_color, included here unchanged).
 *
 *   dsrt_sets_sum_rect   ADDS, for every pixel x in [x0, x1), y in [y0, y1) (y = 0 the bottom row, as the kernel counts), the sums over the samples
 *                        k = first + j*stride (0 <= j < count) of a frame planned at the scene's samples_per_pixel: S (q, units of 2^-20) and, if sum_sq
 *                        is not NULL, S2 (sq = ((uint64)q*q + 2^19) >> 20).  Buffers are width*height*3 uint64 in image order (top row first).
 *   dsrt_sets_resolve    the mean / tone map / rgb8 / f32 of dsrt_oracle_render_rect's mode 1 with spp replaced by samples_done, and the variance of the
 *                        mean in the header's order.  Any output may be NULL.
 *
 * Build: the top-level Makefile, target `oracle` (gcc with the oracle's flags); the library lands next to this file.
 */
#include "../oracle/dsrt_oracle.c"

int dsrt_sets_sum_rect(const GPUScene* s, int W, int H, int x0, int x1, int y0, int y1, int first, int count, int stride, uint64_t* sum, uint64_t* sum_sq) {
    if (!s || !sum || W < 2 || H < 2 || y0 < 0 || y1 > H || y0 > y1 || x0 < 0 || x1 > W || x0 > x1) return -1;
    int spp = s->params.samples_per_pixel;
    if (spp < 1) spp = 1;
    if (first < 0 || count < 1 || stride < 1 || (long long)first + (long long)(count - 1) * stride >= spp) return -1;
    DsrtOracleCounters local;
    memset(&local, 0, sizeof local);
    for (int y = y0; y < y1; ++y) {
        for (int x = x0; x < x1; ++x) {
            const uint64_t pixel = (uint64_t)x + (uint64_t)y * (uint64_t)W;
            const size_t idx = ((size_t)(H - 1 - y) * (size_t)W + (size_t)x) * 3;
            for (int j = 0; j < count; ++j) {
                const int k = first + j * stride;
                Rng g = { .c = &local, .mode = 1, .key0 = (uint32_t)s->seed, .key1 = (uint32_t)(s->seed >> 32), .sub = pixel * (uint64_t)spp + (uint64_t)k };
                float jx = ((float)k + rand01(&g)) / (float)spp;
                float jy = ((float)k + rand01(&g)) / (float)spp;
                Ray ray = camera_ray(&s->camera, x, y, W, H, jx, jy);
                V3 L = ray_color(s, ray, &g, &local);                   /* already clamped to [0,1] */
                const uint32_t q[3] = { dsrt_oracle_mode1_quantize(L.x), dsrt_oracle_mode1_quantize(L.y), dsrt_oracle_mode1_quantize(L.z) };
                for (int ch = 0; ch < 3; ++ch) {
                    sum[idx + ch] += q[ch];
                    if (sum_sq) sum_sq[idx + ch] += (uint32_t)(((uint64_t)q[ch] * q[ch] + (1ull << 19)) >> 20);
                }
            }
        }
    }
    return 0;
}

int dsrt_sets_resolve(const uint64_t* sum, const uint64_t* sum_sq, size_t n_pixels, int samples_done, float gamma, uint8_t* rgb8, float* rgb_f32, float* var) {
    if (!sum || samples_done < 1 || (var && (!sum_sq || samples_done < 2))) return -1;
    const float inv_gamma = 1.0f / (gamma > 0.0f ? gamma : 1.0f);
    const double n = (double)samples_done;
    for (size_t i = 0; i < n_pixels; ++i) {
        float c[3];
        for (int ch = 0; ch < 3; ++ch) {
            const uint64_t S = sum[i * 3 + ch];
            c[ch] = dsrt_oracle_mode1_mean(S, samples_done);
            c[ch] = fmaxf(c[ch], 0.0f);
            c[ch] = fminf(c[ch], 10.0f);
            c[ch] = O_POWF(c[ch], inv_gamma);
            c[ch] = fminf(1.0f, fmaxf(0.0f, c[ch]));                  /* clamp01 */
            if (rgb8) rgb8[i * 3 + ch] = (unsigned char)(255.99f * c[ch]);
            if (rgb_f32) rgb_f32[i * 3 + ch] = c[ch];
            if (var) {
                const double s = (double)S * (1.0 / 1048576.0), s2 = (double)sum_sq[i * 3 + ch] * (1.0 / 1048576.0);
                double v = (s2 - s * s / n) / (n - 1.0);
                v = v > 0.0 ? v : 0.0;
                var[i * 3 + ch] = (float)(v / n);
            }
        }
    }
    return 0;
}
