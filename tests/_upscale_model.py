"""The CPU model of the upscaler (include/dsrt.h, UPSCALER): the header's arithmetic in numpy float32 on whole-image arrays, the taps in the header's order,
every step one correctly rounded IEEE operation (numpy does not contract).  A skipped tap is realised as weight +0: every sum starts at +0 and adding +0 leaves
its bits alone.  Shared by tests/test_upscale_host.py (CPU) and tests/test_gpu_upscale.py, which holds the kernel to it bit for bit.
`bilinear` is the unguided baseline of the quality test: the same raster mapping, 2 x 2 taps -- not code under test."""
import numpy as np

from _denoise_model import F, FLT_MAX, dot

GB_SUN_VISIBLE = 8
GUIDES = ("normal", "position", "albedo", "range")
DEFAULTS = dict(normal_power_log2=5, sigma_z=0.01, sigma_a=0.1, use_sun=1)


def positions(w, h, W, H):
    """(fx (W,), fy (H,)) float32: where the centre of output column X / buffer row Y lies in the low-resolution buffer."""
    fx = ((np.arange(W).astype(F) + F(0.5)) / F(W - 1)) * F(w - 1) - F(0.5)
    fyk = (((H - 1 - np.arange(H)).astype(F) + F(0.5)) / F(H - 1)) * F(h - 1) - F(0.5)
    fy = F(h - 1) - fyk
    return fx.astype(F), fy.astype(F)


def _tent(q, f):
    return np.fmax(F(1) - F(0.5) * np.abs(q.astype(F) - f), F(0))


def upscale(c, v, lo, hi, normal_power_log2=5, sigma_z=0.01, sigma_a=0.1, use_sun=1):
    """(linear, var, support): float32 (H, W, 3), (H, W, 3), (H, W).  c, v: the low-resolution linear colour and its variance (h, w, 3) (v None = zeros);
    lo / hi: the two rasters' guides {"normal", "position", "albedo", "range"[, "flags"]}."""
    c = np.asarray(c, F)
    h, w = c.shape[:2]
    v = np.zeros_like(c) if v is None else np.asarray(v, F)
    Nl, Xl, Al, Rl = (np.asarray(lo[k], F) for k in GUIDES)
    Np, Xp, Ap, R = (np.asarray(hi[k], F) for k in GUIDES)
    H, W = R.shape
    sun = bool(use_sun) and lo.get("flags") is not None and hi.get("flags") is not None
    if sun:
        Fl, Fp = np.asarray(lo["flags"], np.uint8), np.asarray(hi["flags"], np.uint8)
    sz, sa = F(sigma_z), F(sigma_a)
    fx, fy = positions(w, h, W, H)
    x0, y0 = np.floor(fx).astype(np.int64), np.floor(fy).astype(np.int64)
    with np.errstate(all="ignore"):
        den_z = sz * R
        sa2 = sa * sa
        sw1, sw2 = np.zeros((H, W), F), np.zeros((H, W), F)
        sc1, sv1, sc2, sv2 = (np.zeros((H, W, 3), F) for _ in range(4))
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
                cq, vq = c[Q], v[Q]
                # level 2: the tent alone, every tap inside the image
                t2 = np.where(inside, b, F(0))
                sw2 = sw2 + t2
                sc2 = sc2 + np.where(inside[..., None], t2[..., None] * cq, F(0))
                sv2 = sv2 + np.where(inside[..., None], (t2 * t2)[..., None] * vq, F(0))
                # level 1: the guided taps
                ok = inside & (Rl[Q] <= FLT_MAX)
                if sun:
                    ok &= ((Fl[Q] ^ Fp) & GB_SUN_VISIBLE) == 0
                wn = np.fmax(dot(Np, Nl[Q]), F(0))
                for _ in range(normal_power_log2):
                    wn = wn * wn
                ez = np.abs(dot(Np, Xl[Q] - Xp)) / den_z
                da = Al[Q] - Ap
                ea2 = dot(da, da) / sa2
                wt = (b * wn) / ((F(1) + ez * ez) * (F(1) + ea2))
                t1 = np.where(ok, wt, F(0))
                sw1 = sw1 + t1
                sc1 = sc1 + np.where(ok[..., None], t1[..., None] * cq, F(0))
                sv1 = sv1 + np.where(ok[..., None], (t1 * t1)[..., None] * vq, F(0))
        hit = R <= FLT_MAX
        one = hit & (sw1 > 0)
        two = hit & ~one
        lin = np.where(one[..., None], sc1 / sw1[..., None], np.where(two[..., None], sc2 / sw2[..., None], F(0)))
        var = np.where(one[..., None], sv1 / (sw1 * sw1)[..., None], np.where(two[..., None], sv2 / (sw2 * sw2)[..., None], F(0)))
        support = np.where(one, sw1, F(0))
    return lin.astype(F), var.astype(F), support.astype(F)


def bilinear(c, W, H):
    """The unguided baseline: bilinear interpolation of c (h, w, 3) at the same positions, 2 x 2 taps with clamped coordinates."""
    c = np.asarray(c, np.float64)
    h, w = c.shape[:2]
    fx, fy = (a.astype(np.float64) for a in positions(w, h, W, H))
    x0, y0 = np.floor(fx).astype(np.int64), np.floor(fy).astype(np.int64)
    wx, wy = (fx - x0)[None, :, None], (fy - y0)[:, None, None]
    xa, xb, ya, yb = np.clip(x0, 0, w - 1), np.clip(x0 + 1, 0, w - 1), np.clip(y0, 0, h - 1), np.clip(y0 + 1, 0, h - 1)
    top = c[ya][:, xa] * (1 - wx) + c[ya][:, xb] * wx
    bot = c[yb][:, xa] * (1 - wx) + c[yb][:, xb] * wx
    return (top * (1 - wy) + bot * wy).astype(F)


def _unit(a):
    return a / np.sqrt((a * a).sum())


def synthetic_raster(W, H):
    """One raster of a seeded-free synthetic scene that is a function of the pixel-centre ray parameters (u, v) alone, so that two rasters of it are G-buffers of
    one camera: two planes meeting at u = 0.5 (normals perpendicular to them), checker albedo, a disc and a top strip of misses, a slanted sun-shadow edge.
    Returns (guides with "flags", truth (H, W, 3) float64)."""
    ys, xs = np.mgrid[0:H, 0:W]
    u = (xs + 0.5) / (W - 1)
    v = ((H - 1 - ys) + 0.5) / (H - 1)
    left = u < 0.5
    depth = np.where(left, 10.0 + 20.0 * (0.5 - u), 10.0 + 28.0 * (u - 0.5))
    X = np.stack([(u - 0.5) * 4.0, (v - 0.5) * 3.0, -depth], -1)
    nl, nr = _unit(np.cross([4.0, 0.0, 20.0], [0.0, 3.0, 0.0])), _unit(np.cross([4.0, 0.0, -28.0], [0.0, 3.0, 0.0]))
    N = np.where(left[..., None], nl, nr)
    check = ((np.floor(u * 7) + np.floor(v * 5)) % 2)
    A = np.stack([0.3 + 0.5 * check, 0.4 + 0.2 * check, 0.7 - 0.4 * check], -1)
    hit = ((u - 0.8) ** 2 + (v - 0.3) ** 2 > 0.01) & (v < 0.95)
    sunlit = (u + 0.37 * v) < 0.71
    truth = A * np.where(left, 0.8, 0.35)[..., None] * np.where(sunlit, 1.0, 0.25)[..., None] * hit[..., None]
    h3 = hit[..., None]
    guides = {"normal": np.where(h3, N, 0).astype(F), "position": np.where(h3, X, 0).astype(F), "albedo": np.where(h3, A, 0).astype(F),
              "range": np.where(hit, np.sqrt((X * X).sum(-1)), np.inf).astype(F),
              "flags": np.where(hit, 1 | np.where(sunlit, GB_SUN_VISIBLE, 0), 0).astype(np.uint8)}
    return guides, truth


def synthetic_pair(rng, w, h, W, H, noise=0.1):
    """(c, v, lo, hi, truth_hi): a noisy low-resolution linear image of the synthetic scene with a made-up positive variance, the two rasters' guides, and the
    noise-free image at the output resolution."""
    lo, truth_lo = synthetic_raster(w, h)
    hi, truth_hi = synthetic_raster(W, H)
    c = np.clip(truth_lo + noise * rng.standard_normal((h, w, 3)), 0.0, 1.0).astype(F)
    v = (noise * noise * (0.5 + rng.random((h, w, 3)))).astype(F)
    return c, v, lo, hi, truth_hi.astype(F)
