"""The CPU model of the temporal accumulation stage (include/dsrt.h, TEMPORAL ACCUMULATION), on top of tests/_denoise_model.py: the header's arithmetic in numpy
float32 on whole-image arrays, the taps in the header's order, every step one correctly rounded IEEE operation.  A skipped tap leaves every sum as it is
(np.where on the sum, not a zero weight).  Shared by tests/test_temporal_host.py (CPU) and tests/test_gpu_temporal.py, which holds the kernel to it bit for bit."""
import numpy as np

from _denoise_model import F, FLT_MAX, dot, filterable, iterate, start

DEFAULTS = dict(alpha_min=0.1, normal_cos_min=0.9, plane_tol=0.01, min_support=0.9)
CAMERA_FIELDS = ("origin", "lower_left_corner", "horizontal", "vertical", "u", "v", "w")
QNAN = np.array([0x7FC00000], np.uint32).view(F)[0]
INFO = {}


def camera_vectors(cam):
    """{field: float32 (3,)} of a GPUCamera (ctypes) or of a dict that already holds the seven vectors."""
    if isinstance(cam, dict):
        return {k: np.asarray(cam[k], F) for k in CAMERA_FIELDS}
    return {k: np.array([getattr(cam, k).x, getattr(cam, k).y, getattr(cam, k).z], F) for k in CAMERA_FIELDS}


def project(X, cam, W, H):
    """(fx, fy, ok): the header's projection of positions X (..., 3) through the previous camera, before the range test: ok = k > 0 and inside the image test."""
    C = camera_vectors(cam)
    X = np.asarray(X, F)
    with np.errstate(all="ignore"):
        D = X - C["origin"]
        e = C["lower_left_corner"] - C["origin"]
        a, b, cc = dot(D, C["u"]), dot(D, C["v"]), dot(D, C["w"])
        eu, ev, ew = dot(e, C["u"]), dot(e, C["v"]), dot(e, C["w"])
        hu, vv = dot(C["horizontal"], C["u"]), dot(C["vertical"], C["v"])
        k = ew / cc
        s = (a * k - eu) / hu
        t = (b * k - ev) / vv
        fx = s * F(W - 1) - F(0.5)
        fy = F(H - 1) - (t * F(H - 1) - F(0.5))
        ok = (k > 0) & (fx > F(-1)) & (fx < F(W)) & (fy > F(-1)) & (fy < F(H))
    return fx.astype(F), fy.astype(F), ok


def pack_history(c, m, v, N, X):
    """The 16-float records {c, m, v, 0, N, 0, X, 0} as float32 (H, W, 16)."""
    H, W = m.shape
    h = np.zeros((H, W, 16), F)
    h[..., 0:3], h[..., 3], h[..., 4:7], h[..., 8:11], h[..., 12:15] = c, m, v, N, X
    return h


def stage(c, v, n, Fm, guides, prev_cam, prev, alpha_min=0.1, normal_cos_min=0.9, plane_tol=0.01, min_support=0.9):
    """The stage itself: (c', v', m', prev_xy, found) of the Start values (c, v), counts n (int or (H, W)), F_p and the guides; prev = float32 (H, W, 16) or None.
    found: the pixels that blended with history.  INFO (module global) holds the last call's `guarded` and `seen` masks, for the tests."""
    N, X, rng = (np.asarray(guides[k], F) for k in ("normal", "position", "range"))
    H, W = Fm.shape
    nf = np.broadcast_to(np.asarray(n, np.uint32), (H, W)).astype(F)
    prev_xy = np.full((H, W, 2), QNAN, F)
    found = np.zeros((H, W), bool)
    m_out = np.where(Fm, nf, F(0)).astype(F)
    c_out, v_out = c.copy(), v.copy()
    if prev is None:
        return c_out, v_out, m_out, prev_xy, found
    prev = np.asarray(prev, F).reshape(H, W, 16)
    with np.errstate(all="ignore"):
        fx, fy, ok = project(X, prev_cam, W, H)
        projected = ok & (rng <= FLT_MAX)
        prev_xy[..., 0] = np.where(projected, fx, QNAN)
        prev_xy[..., 1] = np.where(projected, fy, QNAN)
        use = projected & Fm
        fxs, fys = np.where(use, fx, F(0)), np.where(use, fy, F(0))          # (indices are formed for the pixels that tap only)
        flx, fly = np.floor(fxs), np.floor(fys)
        x0, y0 = flx.astype(np.int64), fly.astype(np.int64)
        wx, wy = fxs - flx, fys - fly
        ox, oy = F(1) - wx, F(1) - wy
        tol = F(plane_tol) * rng
        sw, sm = np.zeros((H, W), F), np.zeros((H, W), F)
        sc, sv = np.zeros((H, W, 3), F), np.zeros((H, W, 3), F)
        seen = np.zeros((H, W), bool)
        for dx, dy, b in ((0, 0, ox * oy), (1, 0, wx * oy), (0, 1, ox * wy), (1, 1, wx * wy)):
            qx, qy = x0 + dx, y0 + dy
            inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            rec = prev[np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)]
            cq, mq, vq, Nq, Xq = rec[..., 0:3], rec[..., 3], rec[..., 4:7], rec[..., 8:11], rec[..., 12:15]
            take = use & inside & (mq > 0) & (dot(N, Nq) >= F(normal_cos_min)) & (np.abs(dot(N, Xq - X)) <= tol)
            seen |= take & (b >= F(0.99))
            sw = np.where(take, sw + b, sw)
            sc = np.where(take[..., None], sc + b[..., None] * cq, sc)
            sv = np.where(take[..., None], sv + b[..., None] * vq, sv)
            sm = np.where(take, sm + b * mq, sm)
        guarded = np.zeros((H, W), bool)                                          # the occluder guard over the 4 x 4 block around the footprint
        for gy in range(-1, 3):
            for gx in range(-1, 3):
                qx, qy = x0 + gx, y0 + gy
                inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                rec = prev[np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)]
                guarded |= use & inside & (rec[..., 3] > 0) & (dot(N, rec[..., 12:15] - X) > tol)
        found = use & (sw >= F(min_support)) & (seen | ~guarded)
        INFO.update(guarded=guarded, seen=seen, supported=use & (sw >= F(min_support)))
        ch, vh, mh = sc / sw[..., None], sv / sw[..., None], sm / sw
        alpha = np.fmax(nf / (nf + mh), F(alpha_min))
        beta = F(1) - alpha
        cb = beta[..., None] * ch + alpha[..., None] * c
        vb = (beta * beta)[..., None] * vh + (alpha * alpha)[..., None] * v
        c_out = np.where(found[..., None], cb, c).astype(F)
        v_out = np.where(found[..., None], vb, v).astype(F)
        m_out = np.where(found, nf / alpha, m_out).astype(F)
    return c_out, v_out, m_out, prev_xy, found


def denoise_temporal(S, S2, n, guides, prev_cam=None, prev=None, temporal=None, iterations=5, normal_power_log2=5, sigma_l=1.0, sigma_z=0.01, sigma_a=0.1):
    """One frame: {"linear", "var", "next", "prev_xy", "weight", "found", "blended": (c', v')} -- linear / var after `iterations` a-trous iterations on (c', v')."""
    c, v = start(S, S2, n)
    Fm = filterable(guides["range"], n)
    cb, vb, m, prev_xy, found = stage(c, v, n, Fm, guides, prev_cam, prev, **(temporal or DEFAULTS))
    nxt = pack_history(cb, m, vb, np.asarray(guides["normal"], F), np.asarray(guides["position"], F))
    c, v = cb, vb
    for i in range(iterations):
        c, v = iterate(c, v, Fm, guides, 1 << i, normal_power_log2, sigma_l, sigma_z, sigma_a)
    return {"linear": c, "var": v, "next": nxt, "prev_xy": prev_xy, "weight": m, "found": found, "blended": (cb, vb)}


# ---- frames for the tests ----
def exact_camera():
    """A camera of small exact numbers: the point (x, y, -1) projects to s = (x + 1) / 2, t = (y + 1) / 2 with k = 1 and every operation exact, so
    fx = (x + 1) / 2 * (W - 1) - 0.5 can be put exactly on a bound of the image test."""
    return {"origin": (0, 0, 0), "lower_left_corner": (-1, -1, -1), "horizontal": (2, 0, 0), "vertical": (0, 2, 0), "u": (1, 0, 0), "v": (0, 1, 0), "w": (0, 0, 1)}


def pixel_rays(cam, W, H):
    """(origin (3,), directions (H, W, 3)) of the pixel-centre rays in float64, buffer row 0 the top row: the G-buffer's u = (x + 0.5) / (W - 1), v = (ky + 0.5) / (H - 1)."""
    C = {k: v.astype(np.float64) for k, v in camera_vectors(cam).items()}
    rows, xs = np.mgrid[0:H, 0:W]
    u = (xs + 0.5) / (W - 1)
    v = ((H - 1 - rows) + 0.5) / (H - 1)
    d = C["lower_left_corner"] + u[..., None] * C["horizontal"] + v[..., None] * C["vertical"] - C["origin"]
    return C["origin"], d


def wall_frame(rng, cam, W, H, spp=8, miss=0.0):
    """The plane z = 0 seen through `cam`: (S, S2, n, guides) with noisy sums around a random image, X the pixel-centre rays' points on the plane (z exactly 0),
    N = (0, 0, 1) and the range from the camera.  Two such frames of nearby cameras see the same surface: every history tap passes the validity tests."""
    o, d = pixel_rays(cam, W, H)
    t = -o[2] / d[..., 2]
    X = (o + t[..., None] * d)
    X[..., 2] = 0.0
    X = X.astype(F)
    R = np.sqrt(((X.astype(np.float64) - o) ** 2).sum(-1)).astype(F)
    truth = rng.random((H, W, 3)) * 0.8
    S, S2 = np.zeros((H, W, 3), np.uint64), np.zeros((H, W, 3), np.uint64)
    for _ in range(spp):
        q = (np.clip(truth + 0.2 * rng.standard_normal((H, W, 3)), 0, 1) * (1 << 20) + 0.5).astype(np.uint64)
        S += q
        S2 += (q * q + np.uint64(1 << 19)) >> np.uint64(20)
    hit = rng.random((H, W)) >= miss
    N = np.broadcast_to(np.array([0, 0, 1], F), (H, W, 3))
    guides = {"normal": np.where(hit[..., None], N, F(0)).astype(F), "position": np.where(hit[..., None], X, F(0)).astype(F),
              "albedo": np.where(hit[..., None], rng.random((H, W, 3)), 0).astype(F), "range": np.where(hit, R, F(np.inf)).astype(F)}
    return S, S2, np.full((H, W), spp, np.uint32), guides


def random_history(rng, guides, special=0.0):
    """A history of the surface `guides` shows (its own N and X, so taps are valid), with random c, v and weights m in [1, 40).  `special`: the fraction of records
    given one of the values a tap must reject -- m = 0, negative m, NaN m, a NaN normal, an infinite position, a normal turned away, a point off the plane."""
    N, X = np.asarray(guides["normal"], F).copy(), np.asarray(guides["position"], F).copy()
    H, W = N.shape[:2]
    c, v = rng.random((H, W, 3)).astype(F), (rng.random((H, W, 3)) * 1e-2).astype(F)
    m = (1 + 39 * rng.random((H, W))).astype(F)
    kind = np.where(rng.random((H, W)) < special, rng.integers(1, 8, size=(H, W)), 0)
    m[kind == 1] = 0.0
    m[kind == 2] = -3.0
    m[kind == 3] = np.nan
    N[kind == 4] = np.nan
    X[kind == 5] = np.inf
    N[kind == 6] = np.array([0.8, 0, 0.6], F)
    X[kind == 7] += np.array([0, 0, 5], F)
    return pack_history(c, m, v, N, X), kind
