"""The CPU model of the denoiser (include/dsrt.h, DENOISER): the header's arithmetic in numpy float32 on whole-image arrays, the taps in the header's order,
every step one correctly rounded IEEE operation (numpy does not contract).  A skipped tap is realised as weight +0: every sum is >= +0, so adding +0 leaves
its bits alone.  Shared by tests/test_denoise_host.py (CPU) and tests/test_gpu_denoise.py, which holds the kernels to it bit for bit."""
import ctypes as C

import numpy as np

F = np.float32
K3 = (F(0.25), F(0.5), F(0.25))
H5 = (F(0.0625), F(0.25), F(0.375), F(0.25), F(0.0625))
FLT_MAX = np.finfo(np.float32).max
DEFAULTS = dict(iterations=5, normal_power_log2=5, sigma_l=1.0, sigma_z=0.01, sigma_a=0.1)


def lum(x):
    return (F(0.2126) * x[..., 0] + F(0.7152) * x[..., 1]) + F(0.0722) * x[..., 2]


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def start(S, S2, n):
    """(c, v): the mean and the variance of the mean, float32 (H, W, 3), of sums (H, W, 3) uint64 with n samples per pixel (an int, or (H, W) uint32):
    dsrt_resolve_accumulated_counts' arithmetic, in double and converted once; c = +0 for n = 0, v = +0 for n < 2."""
    S, S2 = np.asarray(S, np.uint64), np.asarray(S2, np.uint64)
    cnt = np.broadcast_to(np.asarray(n, np.uint32), S.shape[:2])
    nd = cnt.astype(np.float64)[..., None]
    with np.errstate(all="ignore"):
        unit = np.float64(1.0) / 1048576.0 / nd
        c = np.where(nd > 0, (S.astype(np.float64) * unit).astype(F), F(0))
        s = S.astype(np.float64) * 2.0 ** -20
        s2 = S2.astype(np.float64) * 2.0 ** -20
        var = (s2 - s * s / nd) / (nd - 1.0)
        var = np.where(var > 0, var, 0.0)
        v = np.where(nd >= 2, (var / nd).astype(F), F(0))
    return c.astype(F), v.astype(F)


def filterable(rng, n):
    """F_p = (range_p <= FLT_MAX) && n >= 2; a NaN range compares false."""
    rng = np.asarray(rng, F)
    with np.errstate(invalid="ignore"):
        return (rng <= FLT_MAX) & (np.broadcast_to(np.asarray(n, np.uint32), rng.shape) >= 2)


def iterate(c, v, Fm, guides, step, normal_power_log2, sigma_l, sigma_z, sigma_a):
    """One a-trous iteration: (c', v') from (c, v), both float32 (H, W, 3)."""
    N, X, A, rng = (np.asarray(guides[k], F) for k in ("normal", "position", "albedo", "range"))
    H, W = Fm.shape
    sl, sz, sa = F(sigma_l), F(sigma_z), F(sigma_a)
    with np.errstate(all="ignore"):
        Lv, Lc = lum(v), lum(c)
        g = np.zeros((H, W), F)
        ys, xs = np.arange(H), np.arange(W)
        for ey in (-1, 0, 1):
            qy = np.clip(ys + ey, 0, H - 1)
            for ex in (-1, 0, 1):
                qx = np.clip(xs + ex, 0, W - 1)
                g = g + (K3[ex + 1] * K3[ey + 1]) * Lv[qy][:, qx]
        den_l = sl * np.sqrt(g) + F(2.0 ** -20)
        den_z = sz * rng
        sa2 = sa * sa
        sw = np.zeros((H, W), F)
        sc, sv = np.zeros((H, W, 3), F), np.zeros((H, W, 3), F)
        for dy in range(-2, 3):
            oy = step * dy
            y0, y1 = max(0, -oy), min(H, H - oy)
            if y0 >= y1:
                continue
            for dx in range(-2, 3):
                ox = step * dx
                x0, x1 = max(0, -ox), min(W, W - ox)
                if x0 >= x1:
                    continue
                P = (slice(y0, y1), slice(x0, x1))
                Q = (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
                wn = np.fmax(dot(N[P], N[Q]), F(0))
                for _ in range(normal_power_log2):
                    wn = wn * wn
                ez = np.abs(dot(N[P], X[Q] - X[P])) / den_z[P]
                el = np.abs(Lc[Q] - Lc[P]) / den_l[P]
                da = A[Q] - A[P]
                ea2 = dot(da, da) / sa2
                w = ((H5[dx + 2] * H5[dy + 2]) * wn) / (((F(1) + ez * ez) * (F(1) + el * el)) * (F(1) + ea2))
                ok = Fm[Q]
                w = np.where(ok, w, F(0))
                sw[P] = sw[P] + w
                sc[P] = sc[P] + np.where(ok[..., None], w[..., None] * c[Q], F(0))
                sv[P] = sv[P] + np.where(ok[..., None], (w * w)[..., None] * v[Q], F(0))
        take = (Fm & (sw > 0))[..., None]
        c2 = np.where(take, sc / sw[..., None], c)
        v2 = np.where(take, sv / (sw * sw)[..., None], v)
    return c2.astype(F), v2.astype(F)


def denoise(S, S2, n, guides, iterations=5, normal_power_log2=5, sigma_l=1.0, sigma_z=0.01, sigma_a=0.1, keep=False):
    """(linear, var) float32 (H, W, 3) after `iterations` iterations; with keep, the list of (linear, var) after 0, 1, ... iterations."""
    c, v = start(S, S2, n)
    Fm = filterable(guides["range"], n)
    out = [(c, v)]
    for i in range(iterations):
        c, v = iterate(c, v, Fm, guides, 1 << i, normal_power_log2, sigma_l, sigma_z, sigma_a)
        out.append((c, v))
    return out if keep else (c, v)


def tone_map(linear, gamma, oracle):
    """(rgb8, f32) of a linear image: the resolve's tone map and 8-bit store, pow through the oracle's dsrt_oracle_powf (math_mode 0)."""
    inv_gamma = F(1) / F(gamma if gamma > 0 else 1.0)
    col = np.minimum(np.maximum(np.asarray(linear, F), F(0)), F(10))
    vals, inverse = np.unique(col.view(np.uint32), return_inverse=True)
    powf = oracle.lib.dsrt_oracle_powf
    table = np.array([powf(C.c_float(float(x)), C.c_float(float(inv_gamma))) for x in vals.view(F)], F)
    col = table[inverse].reshape(col.shape)
    col = np.minimum(F(1), np.maximum(F(0), col))
    return (F(255.99) * col).astype(np.uint8), col


def synthetic_frame(rng, W, H, spp=16, miss=0.0, noise=0.3):
    """A seeded synthetic frame: two planes meeting at a vertical edge, checker albedo, `spp` clamped noisy samples per pixel.  Returns (S, S2, n, guides):
    uint64 sums (H, W, 3), uint32 counts (H, W), and the four guide arrays.  `miss`: fraction of pixels whose centre ray misses (range +inf, guides 0)."""
    ys, xs = np.mgrid[0:H, 0:W]
    left = xs < W / 2
    ang = np.where(left, 0.5, -0.7)
    N = np.stack([np.sin(ang), np.zeros_like(ang), np.cos(ang)], -1).astype(F)
    depth = np.where(left, 10.0 + 0.5 * (W / 2 - xs), 10.0 + 0.7 * (xs - W / 2))
    X = np.stack([(xs - W / 2) * 0.1, (H / 2 - ys) * 0.1, -depth], -1).astype(F)
    check = (((xs // 5) + (ys // 4)) % 2).astype(np.float64)
    A = np.stack([0.3 + 0.5 * check, 0.4 + 0.2 * check, 0.7 - 0.4 * check], -1).astype(F)
    rngv = np.sqrt((X.astype(np.float64) ** 2).sum(-1)).astype(F)
    truth = A.astype(np.float64) * np.where(left, 0.8, 0.35)[..., None]
    hit = rng.random((H, W)) >= miss
    S, S2 = np.zeros((H, W, 3), np.uint64), np.zeros((H, W, 3), np.uint64)
    for _ in range(spp):
        q = np.clip((truth + noise * rng.standard_normal((H, W, 3))) * hit[..., None], 0.0, 1.0)
        q = (q * (1 << 20) + 0.5).astype(np.uint64)
        S += q
        S2 += (q * q + np.uint64(1 << 19)) >> np.uint64(20)
    guides = {"normal": np.where(hit[..., None], N, F(0)).astype(F), "position": np.where(hit[..., None], X, F(0)).astype(F),
              "albedo": np.where(hit[..., None], A, F(0)).astype(F), "range": np.where(hit, rngv, F(np.inf)).astype(F)}
    return S, S2, np.full((H, W), spp, np.uint32), guides, (truth * hit[..., None]).astype(F)
