// upscale_pixel_body.h -- the body of upscale_kernel.hip's two gather kernels, included once in each: one output pixel of include/dsrt.h's UPSCALER (HAS_ALPHA false)
// or COVERAGE-AWARE UPSCALER (HAS_ALPHA true).  Not a header: the including kernel defines, before the #include,
//     constexpr bool HAS_ALPHA;   const UpscaleArgs& a;   const float* hi_alpha;   float alpha_min;   uint8_t* out_level     (the last three only looked at with HAS_ALPHA)
// and is a template over DEVICE_LIBM.  The text is included, not called, so that the plain kernel's code is what it was before the coverage form existed,
// instruction for instruction (an inlined function gave the same instructions with commuted operands).
    const int X = (int)blockIdx.x * 16 + (int)(threadIdx.x & 15u), Y = (int)blockIdx.y * 16 + (int)(threadIdx.x >> 4);
    const int W = a.W, H = a.H, w = a.w, h = a.h;
    if (X >= W || Y >= H) return;
    const size_t P = (size_t)Y * (size_t)W + (size_t)X;
    const float R = a.hi_range[P];
    float aP = 1.0f;
    if constexpr (HAS_ALPHA) aP = hi_alpha[P];
    uint32_t level = 0u;

    float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, v0 = 0.0f, v1 = 0.0f, v2 = 0.0f, support = 0.0f;
    if (R <= FLT_MAX && (!HAS_ALPHA || aP > 0.0f)) {                     // false for a miss (+inf) and for a NaN; with coverage, for a pixel no sub-sample hit
        const float fx = (((float)X + 0.5f) / (float)(W - 1)) * (float)(w - 1) - 0.5f;
        const float fyk = (((float)(H - 1 - Y) + 0.5f) / (float)(H - 1)) * (float)(h - 1) - 0.5f;
        const float fy = (float)(h - 1) - fyk;
        const int x0 = (int)floorf(fx), y0 = (int)floorf(fy);
        const float npx = a.hi_normal[P * 3 + 0], npy = a.hi_normal[P * 3 + 1], npz = a.hi_normal[P * 3 + 2];
        const float xpx = a.hi_position[P * 3 + 0], xpy = a.hi_position[P * 3 + 1], xpz = a.hi_position[P * 3 + 2];
        const float apx = a.hi_albedo[P * 3 + 0], apy = a.hi_albedo[P * 3 + 1], apz = a.hi_albedo[P * 3 + 2];
        const bool sun = a.use_sun && a.hi_flags && a.lo_has_flags;
        const uint32_t fp = sun ? (uint32_t)a.hi_flags[P] : 0u;
        const float den_z = a.sigma_z * R;
        const float sa2 = a.sigma_a * a.sigma_a;

        float sw = 0.0f, sc0 = 0.0f, sc1 = 0.0f, sc2 = 0.0f, sv0 = 0.0f, sv1 = 0.0f, sv2 = 0.0f;
        for (int qy = y0 - 1; qy <= y0 + 2; ++qy) {                      // level 1: the guided taps
            if (qy < 0 || qy >= h) continue;
            const float by = fmaxf(1.0f - 0.5f * fabsf((float)qy - fy), 0.0f);
#pragma unroll
            for (int dx = -1; dx <= 2; ++dx) {
                const int qx = x0 + dx;
                if (qx < 0 || qx >= w) continue;
                const size_t q = (size_t)qy * (size_t)w + (size_t)qx;
                const float4 cq = a.cr[q];
                if (!(cq.w <= FLT_MAX)) continue;
                float al = 1.0f;
                if constexpr (HAS_ALPHA) {
                    al = a.nn[q].w;                                      // nn.w: the tap's alpha
                    if (!(al >= alpha_min)) continue;
                }
                const float4 vq = a.vf[q];
                if (sun && ((__float_as_uint(vq.w) ^ fp) & (uint32_t)DSRT_GB_SUN_VISIBLE) != 0u) continue;
                const float4 nq = a.nn[q], xq = a.xx[q], aq = a.aa[q];
                const float bx = fmaxf(1.0f - 0.5f * fabsf((float)qx - fx), 0.0f);
                const float b = bx * by;
                float wn = fmaxf(dot3(npx, npy, npz, nq.x, nq.y, nq.z), 0.0f);
                for (int k = 0; k < a.normal_power_log2; ++k) wn = wn * wn;
                const float ez = fabsf(dot3(npx, npy, npz, xq.x - xpx, xq.y - xpy, xq.z - xpz)) / den_z;
                const float dax = aq.x - apx, day = aq.y - apy, daz = aq.z - apz;
                const float ea2 = dot3(dax, day, daz, dax, day, daz) / sa2;
                if constexpr (HAS_ALPHA) {                               // the covered part's colour and variance, weighed by the share of the samples that made them
                    const float wt = ((b * wn) * al) / ((1.0f + ez * ez) * (1.0f + ea2));
                    const float wt2 = wt * wt, al2 = al * al;
                    sw += wt;
                    sc0 += wt * (cq.x / al); sc1 += wt * (cq.y / al); sc2 += wt * (cq.z / al);
                    sv0 += wt2 * (vq.x / al2); sv1 += wt2 * (vq.y / al2); sv2 += wt2 * (vq.z / al2);
                } else {
                    const float wt = (b * wn) / ((1.0f + ez * ez) * (1.0f + ea2));
                    const float wt2 = wt * wt;
                    sw += wt;
                    sc0 += wt * cq.x; sc1 += wt * cq.y; sc2 += wt * cq.z;
                    sv0 += wt2 * vq.x; sv1 += wt2 * vq.y; sv2 += wt2 * vq.z;
                }
            }
        }
        support = sw;
        bool unmixed = HAS_ALPHA;                                        // the sums are the covered part's: multiplied by the pixel's own alpha below
        if constexpr (HAS_ALPHA) {
            level = 1u;
            if (!(sw > 0.0f)) {                                          // coverage level 2: every usable tap inside the image, the tent times alpha
                sw = 0.0f; sc0 = 0.0f; sc1 = 0.0f; sc2 = 0.0f; sv0 = 0.0f; sv1 = 0.0f; sv2 = 0.0f;
                support = 0.0f;
                level = 2u;
                for (int qy = y0 - 1; qy <= y0 + 2; ++qy) {
                    if (qy < 0 || qy >= h) continue;
                    const float by = fmaxf(1.0f - 0.5f * fabsf((float)qy - fy), 0.0f);
#pragma unroll
                    for (int dx = -1; dx <= 2; ++dx) {
                        const int qx = x0 + dx;
                        if (qx < 0 || qx >= w) continue;
                        const size_t q = (size_t)qy * (size_t)w + (size_t)qx;
                        const float al = a.nn[q].w;
                        if (!(al >= alpha_min)) continue;
                        const float4 cq = a.cr[q], vq = a.vf[q];
                        const float bx = fmaxf(1.0f - 0.5f * fabsf((float)qx - fx), 0.0f);
                        const float wt = (bx * by) * al;
                        const float wt2 = wt * wt, al2 = al * al;
                        sw += wt;
                        sc0 += wt * (cq.x / al); sc1 += wt * (cq.y / al); sc2 += wt * (cq.z / al);
                        sv0 += wt2 * (vq.x / al2); sv1 += wt2 * (vq.y / al2); sv2 += wt2 * (vq.z / al2);
                    }
                }
                if (!(sw > 0.0f)) { level = 3u; unmixed = false; }
            }
        }
        if (!(sw > 0.0f)) {                                              // level 2 (coverage level 3): every tap inside the image, the tent alone
            sw = 0.0f; sc0 = 0.0f; sc1 = 0.0f; sc2 = 0.0f; sv0 = 0.0f; sv1 = 0.0f; sv2 = 0.0f;
            support = 0.0f;
            for (int qy = y0 - 1; qy <= y0 + 2; ++qy) {
                if (qy < 0 || qy >= h) continue;
                const float by = fmaxf(1.0f - 0.5f * fabsf((float)qy - fy), 0.0f);
#pragma unroll
                for (int dx = -1; dx <= 2; ++dx) {
                    const int qx = x0 + dx;
                    if (qx < 0 || qx >= w) continue;
                    const size_t q = (size_t)qy * (size_t)w + (size_t)qx;
                    const float4 cq = a.cr[q], vq = a.vf[q];
                    const float bx = fmaxf(1.0f - 0.5f * fabsf((float)qx - fx), 0.0f);
                    const float wt = bx * by;
                    const float wt2 = wt * wt;
                    sw += wt;
                    sc0 += wt * cq.x; sc1 += wt * cq.y; sc2 += wt * cq.z;
                    sv0 += wt2 * vq.x; sv1 += wt2 * vq.y; sv2 += wt2 * vq.z;
                }
            }
        }
        const float sw2 = sw * sw;
        c0 = sc0 / sw; c1 = sc1 / sw; c2 = sc2 / sw;
        v0 = sv0 / sw2; v1 = sv1 / sw2; v2 = sv2 / sw2;
        if constexpr (HAS_ALPHA) {
            if (unmixed) {
                const float aP2 = aP * aP;
                c0 = c0 * aP; c1 = c1 * aP; c2 = c2 * aP;
                v0 = v0 * aP2; v1 = v1 * aP2; v2 = v2 * aP2;
            }
        }
    }

    if (a.out_linear) { a.out_linear[P * 3 + 0] = c0; a.out_linear[P * 3 + 1] = c1; a.out_linear[P * 3 + 2] = c2; }
    if (a.out_var) { a.out_var[P * 3 + 0] = v0; a.out_var[P * 3 + 1] = v1; a.out_var[P * 3 + 2] = v2; }
    if (a.out_support) a.out_support[P] = support;
    if constexpr (HAS_ALPHA) { if (out_level) out_level[P] = (uint8_t)level; }
    if (!a.out_rgb8 && !a.out_f32) return;
    const F3 col = mk(tone_map<DEVICE_LIBM>(c0, a.inv_gamma), tone_map<DEVICE_LIBM>(c1, a.inv_gamma), tone_map<DEVICE_LIBM>(c2, a.inv_gamma));
    if (a.out_rgb8) store_rgb8(a.out_rgb8, P * 3, col);
    if (a.out_f32) { a.out_f32[P * 3 + 0] = col.x; a.out_f32[P * 3 + 1] = col.y; a.out_f32[P * 3 + 2] = col.z; }
