"""The CPU model of the lens stage (include/dsrt.h, LENS MODEL): the header's arithmetic in numpy float32 on whole-image arrays, one correctly rounded IEEE
operation per line, the taps in the header's order; a skipped tap leaves the sum as it is (np.where on the sum, not a zero weight).  Shared by
tests/test_lens_host.py (CPU), which holds dsrt_lens_distort_points to it, and tests/test_gpu_lens.py, which holds the kernel to it bit for bit.  `reference64`
is the same formulas in float64, for the model's own error."""
import numpy as np

F = np.float32
ITERATIONS = 12
CERTIFICATE = F(2.0 ** -6)
NEAREST, BILINEAR, CUBIC = 0, 1, 2
INVERTED, ANY_TAP, ALL_TAPS = 1, 2, 4
TAPS = {NEAREST: 1, BILINEAR: 2, CUBIC: 4}

DEFAULTS = dict(src_width=0, src_height=0, src_fx=0.0, src_fy=0.0, src_cx=0.0, src_cy=0.0, fx=0.0, fy=0.0, cx=0.0, cy=0.0, k1=0.0, k2=0.0, k3=0.0, p1=0.0, p2=0.0,
                v1=0.0, v2=0.0, v3=0.0, cos4=0, filter=CUBIC, channels=3, clamp_zero=1, fill_bits=0)
FLOAT_FIELDS = ("src_fx", "src_fy", "src_cx", "src_cy", "fx", "fy", "cx", "cy", "k1", "k2", "k3", "p1", "p2", "v1", "v2", "v3")


def centred(W, H, sw, sh, f, src_f=None, **coeffs):
    """Parameters for an output of W x H from a source of sw x sh, both principal points at the frames' centres ((size - 1) / 2), focal lengths f and src_f (default f)."""
    src_f = f if src_f is None else src_f
    return dict(src_width=sw, src_height=sh, src_fx=src_f, src_fy=src_f, src_cx=(sw - 1) / 2, src_cy=(sh - 1) / 2, fx=f, fy=f, cx=(W - 1) / 2, cy=(H - 1) / 2, **coeffs)


# The test shapes: name -> (W, H, parameters without filter and channels).  The smallest at which tile seams (64 x 4 output pixels per workgroup), partial waves, the
# fold-over and the border taps all occur.
CASES = {
    "barrel": (37, 21, centred(37, 21, 45, 29, 30.0, k1=-0.25, k2=0.05, p1=0.002, p2=-0.001)),
    "pincushion": (37, 21, centred(37, 21, 45, 29, 30.0, k1=0.2, k2=0.05, k3=0.01)),
    "mixed": (37, 21, centred(37, 21, 33, 17, 30.0, k1=-0.9, p1=0.01, p2=-0.01)),
    "wide": (130, 9, centred(130, 9, 70, 19, 60.0, src_f=30.0, k1=-0.25, k2=0.05, p1=0.002, p2=-0.001)),
    "tiny": (2, 2, centred(2, 2, 2, 2, 30.0, k1=-0.25, k2=0.05, p1=0.002, p2=-0.001)),
}


def params(**changes):
    """The model's parameters: DEFAULTS (dsrt_lens_defaults) with `changes` applied, the float fields as float32."""
    unknown = set(changes) - set(DEFAULTS)
    assert not unknown, unknown
    p = dict(DEFAULTS, **changes)
    for k in FLOAT_FIELDS:
        p[k] = F(p[k])
    return p


def terms(p, xu, yu):
    """rad, dx, dy of the forward model at (xu, yu): step 2."""
    xx = xu * xu
    yy = yu * yu
    xy = xu * yu
    r2 = xx + yy
    t = r2 * p["k3"]
    t = p["k2"] + t
    t = r2 * t
    t = p["k1"] + t
    t = r2 * t
    rad = F(1) + t
    two_p1 = F(2) * p["p1"]
    two_p2 = F(2) * p["p2"]
    a = two_p1 * xy
    b = F(2) * xx
    b = r2 + b
    b = p["p2"] * b
    dx = a + b
    c = F(2) * yy
    c = r2 + c
    c = p["p1"] * c
    d = two_p2 * xy
    dy = c + d
    return rad, dx, dy


def distort(p, xu, yu):
    rad, dx, dy = terms(p, xu, yu)
    xr = xu * rad
    xr = xr + dx
    yr = yu * rad
    yr = yr + dy
    return xr, yr


def undistort(p, xd, yd):
    """Step 3: exactly ITERATIONS fixed-point steps, both coordinates from the previous pair."""
    xu, yu = xd, yd
    for _ in range(ITERATIONS):
        rad, dx, dy = terms(p, xu, yu)
        xn = xd - dx
        xn = xn / rad
        yn = yd - dy
        yn = yn / rad
        xu, yu = xn, yn
    return xu, yu


def certified(p, xu, yu, xd, yd):
    xr, yr = distort(p, xu, yu)
    ex = xr - xd
    ex = np.abs(ex * p["fx"])
    ey = yr - yd
    ey = np.abs(ey * p["fy"])
    return (ex <= CERTIFICATE) & (ey <= CERTIFICATE)                 # a NaN fails


def in_window(s, size):
    return (s > F(-3)) & (s < F(size) + F(2))                        # a NaN fails


def cubic_weights(t):
    w0 = F(-0.5) * t
    w0 = w0 + F(1)
    w0 = w0 * t
    w0 = w0 - F(0.5)
    w0 = w0 * t
    w1 = F(1.5) * t
    w1 = w1 - F(2.5)
    w1 = w1 * t
    w1 = w1 * t
    w1 = w1 + F(1)
    w2 = F(-1.5) * t
    w2 = w2 + F(2)
    w2 = w2 * t
    w2 = w2 + F(0.5)
    w2 = w2 * t
    w3 = F(0.5) * t
    w3 = w3 - F(0.5)
    w3 = w3 * t
    w3 = w3 * t
    return [w0, w1, w2, w3]


def vignette(p, xu, yu):
    a = xu * xu
    b = yu * yu
    ru2 = a + b
    g = ru2 * p["v3"]
    g = p["v2"] + g
    g = ru2 * g
    g = p["v1"] + g
    g = ru2 * g
    g = F(1) + g
    if p["cos4"]:
        q = F(1) + ru2
        q = q * q
        g = g / q
    return np.fmax(g, F(0))


def positions(p, W, H):
    """Steps 1 to 5 for the whole output frame: (xu, yu, inverted, sx, sy, taps), arrays (H, W)."""
    ys, xs = np.mgrid[0:H, 0:W]
    with np.errstate(all="ignore"):
        xd = xs.astype(F) - p["cx"]
        xd = xd / p["fx"]
        yd = ys.astype(F) - p["cy"]
        yd = yd / p["fy"]
        xu, yu = undistort(p, xd, yd)
        inverted = certified(p, xu, yu, xd, yd)
        sx = xu * p["src_fx"]
        sx = sx + p["src_cx"]
        sy = yu * p["src_fy"]
        sy = sy + p["src_cy"]
        taps = inverted & in_window(sx, p["src_width"]) & in_window(sy, p["src_height"])
    return xu, yu, inverted, sx, sy, taps


def apply(p, src, W, H):
    """The whole contract: {image, src_xy, status} for the source `src` (src_height, src_width, channels) -- float32 for filters 1 and 2, any 32-bit dtype for
    nearest -- and the output size W x H.  image has src's dtype and shape (H, W, channels)."""
    sw, sh, C, flt = p["src_width"], p["src_height"], p["channels"], p["filter"]
    src = np.ascontiguousarray(src).reshape(sh, sw, C)
    assert src.dtype.itemsize == 4 and (flt == NEAREST or src.dtype == F)
    xu, yu, inverted, sx, sy, taps = positions(p, W, H)
    n = TAPS[flt]
    n_inside = np.zeros((H, W), np.int64)
    with np.errstate(all="ignore"):
        sxs, sys_ = np.where(taps, sx, F(0)), np.where(taps, sy, F(0))          # (indices are formed for the pixels that tap only)
        if flt == NEAREST:
            qx = np.floor(sxs + F(0.5)).astype(np.int64)
            qy = np.floor(sys_ + F(0.5)).astype(np.int64)
            inside = taps & (qx >= 0) & (qx < sw) & (qy >= 0) & (qy < sh)
            words = src.view(np.uint32)[np.clip(qy, 0, sh - 1), np.clip(qx, 0, sw - 1)]
            image = np.where(inside[..., None], words, np.uint32(p["fill_bits"])).astype(np.uint32)
            n_inside += inside
        else:
            fx0, fy0 = np.floor(sxs), np.floor(sys_)
            tx, ty = sxs - fx0, sys_ - fy0
            if flt == BILINEAR:
                wx, wy = [F(1) - tx, tx], [F(1) - ty, ty]
            else:
                wx, wy = cubic_weights(tx), cubic_weights(ty)
            x0 = fx0.astype(np.int64) - (1 if n == 4 else 0)
            y0 = fy0.astype(np.int64) - (1 if n == 4 else 0)
            acc = np.zeros((H, W, C), F)
            for j in range(n):
                for i in range(n):
                    qx, qy = x0 + i, y0 + j
                    inside = taps & (qx >= 0) & (qx < sw) & (qy >= 0) & (qy < sh)
                    c = src[np.clip(qy, 0, sh - 1), np.clip(qx, 0, sw - 1)]
                    w = wy[j] * wx[i]
                    term = w[..., None] * c
                    acc = np.where(inside[..., None], acc + term, acc)
                    n_inside += inside
            g = vignette(p, xu, yu)
            out = acc * g[..., None]
            if p["clamp_zero"]:
                out = np.fmax(out, F(0))
            image = np.where(inverted[..., None], out, F(0)).astype(F).view(np.uint32)
    status = (inverted * INVERTED | (n_inside > 0) * ANY_TAP | (n_inside == n * n) * ALL_TAPS).astype(np.uint8)
    src_xy = np.where(inverted[..., None], np.stack([sx, sy], axis=-1), F(0)).astype(F)
    return {"image": image.view(src.dtype), "src_xy": src_xy, "status": status}


def distort_points(p, xy):
    """dsrt_lens_distort_points: (xy_out (N, 2) float32, ok (N,) uint8)."""
    xy = np.asarray(xy, F).reshape(-1, 2)
    with np.errstate(all="ignore"):
        xu = xy[:, 0] - p["src_cx"]
        xu = xu / p["src_fx"]
        yu = xy[:, 1] - p["src_cy"]
        yu = yu / p["src_fy"]
        xr, yr = distort(p, xu, yu)
        ox = xr * p["fx"]
        ox = ox + p["cx"]
        oy = yr * p["fy"]
        oy = oy + p["cy"]
        ok = np.isfinite(xy).all(axis=1) & np.isfinite(ox) & np.isfinite(oy)
    out = np.where(ok[:, None], np.stack([ox, oy], axis=1), F(0)).astype(F)
    return out, ok.astype(np.uint8)


def reference64(p, W, H):
    """Steps 1 to 5 with the same formulas and the same twelve steps in float64, from the float32 parameters: (xu, yu, sx, sy)."""
    q = {k: (np.float64(v) if k in FLOAT_FIELDS else v) for k, v in p.items()}
    ys, xs = np.mgrid[0:H, 0:W]
    xd = (xs - q["cx"]) / q["fx"]
    yd = (ys - q["cy"]) / q["fy"]

    def terms64(xu, yu):
        r2 = xu * xu + yu * yu
        rad = 1 + r2 * (q["k1"] + r2 * (q["k2"] + r2 * q["k3"]))
        dx = 2 * q["p1"] * xu * yu + q["p2"] * (r2 + 2 * xu * xu)
        dy = q["p1"] * (r2 + 2 * yu * yu) + 2 * q["p2"] * xu * yu
        return rad, dx, dy

    xu, yu = xd, yd
    with np.errstate(all="ignore"):
        for _ in range(ITERATIONS):
            rad, dx, dy = terms64(xu, yu)
            xu, yu = (xd - dx) / rad, (yd - dy) / rad
    return xu, yu, xu * q["src_fx"] + q["src_cx"], yu * q["src_fy"] + q["src_cy"]
