"""The CPU model of the upscaler with coverage (include/dsrt.h, COVERAGE-AWARE UPSCALER): the header's arithmetic in numpy float32 on whole-image arrays, the
taps in the header's order, every step one correctly rounded IEEE operation (numpy does not contract).  As in tests/_upscale_model.py a skipped tap is realised as
weight +0: every sum starts at +0 and adding +0 leaves its bits alone.  Shared by tests/test_upscale_coverage_host.py (CPU) and
tests/test_gpu_upscale_coverage.py, which holds the kernel to it bit for bit, the level byte included."""
import numpy as np

from _denoise_model import F, FLT_MAX, dot
from _upscale_model import GB_SUN_VISIBLE, GUIDES, _tent, positions, upscale

ALPHA_MIN = 0.125                                                                    # dsrt_upscale_coverage_alpha_min(): the chain's default, for its denoiser too


def upscale_coverage(c, v, lo, hi, alpha_lo, alpha_hi, alpha_min=ALPHA_MIN, normal_power_log2=5, sigma_z=0.01, sigma_a=0.1, use_sun=1):
    """(linear, var, support, level): float32 (H, W, 3), (H, W, 3), (H, W) and uint8 (H, W).  c, v, lo, hi as _upscale_model.upscale; alpha_lo (h, w) and alpha_hi
    (H, W) the two rasters' coverage.  Both None is the plain upscaler (identity 1), with its levels named as the header names them: 0, 1 and 3."""
    if alpha_lo is None and alpha_hi is None:
        lin, var, sup = upscale(c, v, lo, hi, normal_power_log2, sigma_z, sigma_a, use_sun)
        with np.errstate(invalid="ignore"):
            hit = np.asarray(hi["range"], F) <= FLT_MAX
        return lin, var, sup, np.where(~hit, 0, np.where(sup > 0, 1, 3)).astype(np.uint8)
    assert alpha_lo is not None and alpha_hi is not None, "the two alphas go together"
    c = np.asarray(c, F)
    h, w = c.shape[:2]
    v = np.zeros_like(c) if v is None else np.asarray(v, F)
    Nl, Xl, Al, Rl = (np.asarray(lo[k], F) for k in GUIDES)
    Np, Xp, Ap, R = (np.asarray(hi[k], F) for k in GUIDES)
    H, W = R.shape
    al, aP = np.asarray(alpha_lo, F).reshape(h, w), np.asarray(alpha_hi, F).reshape(H, W)
    sun = bool(use_sun) and lo.get("flags") is not None and hi.get("flags") is not None
    if sun:
        Fl, Fp = np.asarray(lo["flags"], np.uint8), np.asarray(hi["flags"], np.uint8)
    sz, sa, amin = F(sigma_z), F(sigma_a), F(alpha_min)
    fx, fy = positions(w, h, W, H)
    x0, y0 = np.floor(fx).astype(np.int64), np.floor(fy).astype(np.int64)
    with np.errstate(all="ignore"):
        den_z = sz * R
        sa2 = sa * sa
        sw1, sw2, sw3 = (np.zeros((H, W), F) for _ in range(3))
        sc1, sv1, sc2, sv2, sc3, sv3 = (np.zeros((H, W, 3), F) for _ in range(6))
        for dy in range(-1, 3):
            qy = y0 + dy
            iny = (qy >= 0) & (qy < h)
            by = _tent(qy, fy)
            qyc = np.clip(qy, 0, h - 1)
            for dx in range(-1, 3):
                qx = x0 + dx
                inx = (qx >= 0) & (qx < w)
                bx = _tent(qx, fx)
                qxc = np.clip(qx, 0, w - 1)
                Q = (qyc[:, None], qxc[None, :])
                inside = iny[:, None] & inx[None, :]
                b = bx[None, :] * by[:, None]
                cq, vq, a = c[Q], v[Q], al[Q]
                usable = inside & (a >= amin)                                        # a NaN alpha compares false
                u = cq / a[..., None]
                aa = a * a
                vu = vq / aa[..., None]
                # level 3: UPSCALER's level 2 -- the tent alone, every tap inside the image, the mixed colour
                t3 = np.where(inside, b, F(0))
                sw3 = sw3 + t3
                sc3 = sc3 + np.where(inside[..., None], t3[..., None] * cq, F(0))
                sv3 = sv3 + np.where(inside[..., None], (t3 * t3)[..., None] * vq, F(0))
                # level 2: the tent times alpha, every usable tap inside the image, the unmixed colour
                t2 = np.where(usable, b * a, F(0))
                sw2 = sw2 + t2
                sc2 = sc2 + np.where(usable[..., None], t2[..., None] * u, F(0))
                sv2 = sv2 + np.where(usable[..., None], (t2 * t2)[..., None] * vu, F(0))
                # level 1: the guided taps
                ok = usable & (Rl[Q] <= FLT_MAX)
                if sun:
                    ok &= ((Fl[Q] ^ Fp) & GB_SUN_VISIBLE) == 0
                wn = np.fmax(dot(Np, Nl[Q]), F(0))
                for _ in range(normal_power_log2):
                    wn = wn * wn
                ez = np.abs(dot(Np, Xl[Q] - Xp)) / den_z
                da = Al[Q] - Ap
                ea2 = dot(da, da) / sa2
                wt = ((b * wn) * a) / ((F(1) + ez * ez) * (F(1) + ea2))
                t1 = np.where(ok, wt, F(0))
                sw1 = sw1 + t1
                sc1 = sc1 + np.where(ok[..., None], t1[..., None] * u, F(0))
                sv1 = sv1 + np.where(ok[..., None], (t1 * t1)[..., None] * vu, F(0))
        live = (R <= FLT_MAX) & (aP > 0)
        one = live & (sw1 > 0)
        two = live & ~one & (sw2 > 0)
        three = live & ~one & ~two
        aP2 = aP * aP
        lin = np.where(one[..., None], (sc1 / sw1[..., None]) * aP[..., None],
                       np.where(two[..., None], (sc2 / sw2[..., None]) * aP[..., None], np.where(three[..., None], sc3 / sw3[..., None], F(0))))
        var = np.where(one[..., None], (sv1 / (sw1 * sw1)[..., None]) * aP2[..., None],
                       np.where(two[..., None], (sv2 / (sw2 * sw2)[..., None]) * aP2[..., None], np.where(three[..., None], sv3 / (sw3 * sw3)[..., None], F(0))))
        support = np.where(one, sw1, F(0))
        level = np.where(one, 1, np.where(two, 2, np.where(three, 3, 0))).astype(np.uint8)
    return lin.astype(F), var.astype(F), support.astype(F), level


def synthetic_alphas(rng, lo, hi, alpha_min=ALPHA_MIN):
    """(alpha_lo, alpha_hi) for a synthetic pair's guides: mostly a smooth coverage in [0.3, 1], 1 and 0 in stripes, and every value that takes another path
    scattered over both rasters -- 0, 1, just below and just above alpha_min, alpha_min itself, 1/64 and NaN.  The low-resolution raster also gets a block of
    unusable pixels large enough that some output pixels find no usable tap at all (level 3), unless the raster is too small to hold one."""
    below, above = np.nextafter(F(alpha_min), F(0)), np.nextafter(F(alpha_min), F(1))
    special = np.array([0.0, 1.0, below, above, alpha_min, 1 / 64, np.nan], F)
    out = []
    for g in (lo, hi):
        H, W = g["range"].shape
        ys, xs = np.mgrid[0:H, 0:W]
        a = (0.65 + 0.35 * np.sin(0.9 * xs + 0.5 * ys)).astype(F)
        a[(xs + 2 * ys) % 11 == 0] = 1.0
        a[(3 * xs + ys) % 13 == 0] = 0.0
        pick = rng.random((H, W)) < 0.15
        a[pick] = special[rng.integers(0, special.size, int(pick.sum()))]
        out.append(a)
    h, w = out[0].shape
    if h >= 12 and w >= 12:
        out[0][h // 3:h // 3 + 6, w // 4:w // 4 + 6] = below
    return out[0], out[1]
