"""The CPU model of the star field (include/dsrt.h, POINT SOURCES): the header's arithmetic in numpy float32, one correctly rounded IEEE operation at a time, the
deposits summed as integers with np.add.at.  `blocked` -- step 2 -- is not modelled here: it is the boolean of the oracle's scene_hit for the ray (C.origin, D),
which `blocked_by_oracle` asks through the helpers of tests/test_gpu_trace_rays.py.  Shared by tests/test_stars_host.py (CPU) and tests/test_gpu_stars.py, which
holds the kernels to it bit for bit."""
import numpy as np

from _denoise_model import F, dot
from _temporal_model import camera_vectors

PROJECTED, VISIBLE, INSIDE = 1, 2, 4
QUANTA = F(16777216.0)           # 2^24
CAP = F(1099511627776.0)         # 2^40
SCALE = F(2.0) ** F(-24)


def u64_to_f32(A):
    """(float)A of uint64 sums: numpy's cast, which rounds to nearest even in one step (tests/test_stars_host.py pins it against u64_to_f32_by_integers)."""
    return np.asarray(A, np.uint64).astype(F)


def u64_to_f32_by_integers(a):
    """The float32 nearest the integer a (0 <= a < 2^64), ties to even, by integer arithmetic alone."""
    a = int(a)
    if a == 0:
        return F(0.0)
    e = a.bit_length() - 1                   # a in [2^e, 2^(e+1))
    if e <= 23:
        return np.array([(e + 127) << 23 | ((a << (23 - e)) & 0x7FFFFF)], np.uint32).view(F)[0]
    shift = e - 23
    m, rest, half = a >> shift, a & ((1 << shift) - 1), 1 << (shift - 1)
    if rest > half or (rest == half and (m & 1)):
        m += 1
        if m == 1 << 24:
            m, e = 1 << 23, e + 1
    return np.array([(e + 127) << 23 | (m & 0x7FFFFF)], np.uint32).view(F)[0]


def project(D, cam, W, H):
    """(fx, fy, projected) of the directions D (N, 3): TEMPORAL ACCUMULATION's projection with D in place of X_p - C.origin."""
    C = camera_vectors(cam)
    D = np.asarray(D, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
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


def blocked_by_oracle(oracle, scene, D, which=None):
    """Step 2 for the stars `which` (a boolean mask; None: all): scene_hit(ray(C.origin, D), 0.001f, 1e9f) of the CPU oracle, as a boolean array over all stars."""
    import ctypes as C
    from test_gpu_gbuffer import _oracle_lib
    L = _oracle_lib(oracle)
    D = np.ascontiguousarray(D, F).reshape(-1, 3)
    o = scene.camera.origin
    o3 = (C.c_float * 3)(o.x, o.y, o.z)
    out, ids = (C.c_float * 9)(), (C.c_int * 4)()
    fp = C.POINTER(C.c_float)
    blocked = np.zeros(len(D), bool)
    for i in (range(len(D)) if which is None else np.nonzero(which)[0]):
        blocked[i] = bool(L.dsrt_oracle_scene_hit(C.byref(scene), o3, D[i].ctypes.data_as(fp), 0.001, 1e9, out, ids))
    return blocked


def deposits(flux, fx, fy, visible, W, H):
    """Step 3: the accumulator A, uint64 (H, W, 3), and per star whether all four taps lie inside the image."""
    flux = np.asarray(flux, F).reshape(-1, 3)
    A = np.zeros((H, W, 3), np.uint64)
    with np.errstate(all="ignore"):
        x0f, y0f = np.floor(fx), np.floor(fy)
        wx, wy = fx - x0f, fy - y0f
        ox, oy = F(1) - wx, F(1) - wy
        finite = np.isfinite(x0f) & np.isfinite(y0f)
        x0 = np.where(finite, x0f, -9).astype(np.int64)
        y0 = np.where(finite, y0f, -9).astype(np.int64)
        inside = (x0 >= 0) & (x0 + 1 < W) & (y0 >= 0) & (y0 + 1 < H)
        for q, bq in enumerate((ox * oy, wx * oy, ox * wy, wx * wy)):
            qx, qy = x0 + (q & 1), y0 + (q >> 1)
            take = visible & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            for k in range(3):
                d = (flux[:, k] * bq).astype(F)
                qf = np.fmin(np.fmax((d * QUANTA).astype(F), F(0)), CAP)
                n = np.where(take, qf, F(0)).astype(np.uint64)          # truncation; 0 <= qf <= 2^40
                np.add.at(A, (qy[take], qx[take], k), n[take])
    return A, inside


def render(D, flux, cam, W, H, blocked=None, linear=None):
    """The whole contract: {layer, linear_out (with `linear`), xy, status, A}.  blocked: boolean per star (None: occlusion == 0)."""
    fx, fy, proj = project(D, cam, W, H)
    vis = proj if blocked is None else proj & ~np.asarray(blocked, bool)
    A, inside = deposits(flux, fx, fy, vis, W, H)
    layer = (u64_to_f32(A) * SCALE).astype(F)
    out = {"A": A, "layer": layer}
    out["xy"] = np.where(proj[:, None], np.stack([fx, fy], axis=1), F(0)).astype(F)
    out["status"] = (proj * PROJECTED | vis * VISIBLE | (proj & inside) * INSIDE).astype(np.uint8)
    if linear is not None:
        out["linear_out"] = (np.asarray(linear, F).reshape(H, W, 3) + layer).astype(F)
    return out
