"""The lens model's specification (include/dsrt.h, LENS MODEL) where it does not depend on the kernel: the numpy model of tests/_lens_model.py -- identity, the
round trip through the forward model, its own error against float64 -- and the host half of the library: dsrt_lens_distort_points bit for bit against the model,
ABI, defaults, every refusal (dsrt_lens_apply looks at its context last, so a machine without a device sees all the others), the pinhole's intrinsics and the
CLI's usage errors.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import _lens_model as M
from _lens_model import F
from _temporal_model import pixel_rays

NEW_NAMES = ("DsrtLens", "DsrtLensOut", "dsrt_lens_defaults", "dsrt_lens_apply", "dsrt_lens_apply_to_host", "dsrt_lens_distort_points",
             "dsrt_lens_intrinsics_from_camera", "DSRT_SIZEOF_LENS", "DSRT_SIZEOF_LENS_OUT")
FUNCTIONS = tuple(n for n in NEW_NAMES if n.startswith("dsrt_"))
EXE = os.path.join(ROOT, "deep-space-ray-tracer_amd", "dsrt_render")
EPS = 2.0 ** -24                                                    # fp32's unit roundoff: one correctly rounded operation is off by at most EPS * |result|


def lib_params(dsrt, p):
    """The DsrtLens of the model's parameter dict."""
    return dsrt.lens_defaults(**{k: (float(v) if k in M.FLOAT_FIELDS else int(v)) for k, v in p.items()})


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- 1. the point helper against the model ----
def test_distort_points_match_the_model_bit_for_bit(dsrt):
    rng = np.random.default_rng(21)
    inf, nan = np.inf, np.nan
    for name in ("barrel", "pincushion", "mixed", "wide"):
        W, H, kw = M.CASES[name]
        p = M.params(**kw)
        sw, sh = p["src_width"], p["src_height"]
        inside = rng.uniform((-1.0, -1.0), (sw, sh), (3000, 2))
        far = rng.uniform(-1.0, 1.0, (600, 2)) * 10.0 ** rng.uniform(2, 30, (600, 1))      # far outside the frame, up to where the polynomial overflows
        grid = np.stack(np.meshgrid(np.arange(sw), np.arange(sh)), axis=-1).reshape(-1, 2)
        special = np.array([[nan, 1], [1, nan], [inf, 1], [1, -inf], [inf, inf], [nan, nan], [3e38, 3e38], [-0.0, 0.0], [1e-40, -1e-40], [p["src_cx"], p["src_cy"]]])
        xy = np.concatenate([inside, far, grid, special]).astype(F)
        got, ok = dsrt.lens_distort_points(lib_params(dsrt, p), xy)
        want, want_ok = M.distort_points(p, xy)
        assert np.array_equal(ok, want_ok) and np.array_equal(bits(got), bits(want)), name
        assert ok[:3000].all() and not ok[-10:-3].any() and ok[-3:].all()                      # the non-finite inputs, and 3e38 (it overflows), are not ok
        assert 0 < (ok[3000:3600] == 0).sum() < 600, "the far points should overflow in part"
        assert not got[ok == 0].view(np.uint32).any()                                          # ... and come out as +0
        assert np.array_equal(got[-1], np.array([p["cx"], p["cy"]], F))                        # the principal point maps to the principal point


def test_distort_points_refusals(dsrt):
    L = dsrt.lib
    good = lib_params(dsrt, M.params(**M.CASES["barrel"][2]))
    xy, out, ok = np.ones(4, F), np.full(4, 7.0, F), np.full(2, 9, np.uint8)
    call = lambda p, n=2, a=xy, b=out: L.dsrt_lens_distort_points(C.byref(p) if p is not None else None, n, a.ctypes.data if a is not None else None,      # noqa: E731
                                                                  b.ctypes.data if b is not None else None, ok.ctypes.data)
    assert call(None) == -1 and call(good, -1) == -1 and call(good, 2, None) == -1 and call(good, 2, xy, None) == -1
    assert call(good, 0, None, None) == 0                                                       # no points: nothing to read or write
    for field, values in (("fx", (0.0, -1.0, np.nan, np.inf)), ("fy", (0.0, np.nan)), ("src_fx", (0.0, -2.0, np.inf)), ("src_fy", (np.nan,)),
                          ("cx", (np.nan, np.inf)), ("cy", (-np.inf,)), ("src_cx", (np.nan,)), ("src_cy", (np.inf,)),
                          ("k1", (np.nan, np.inf)), ("k2", (np.nan,)), ("k3", (-np.inf,)), ("p1", (np.nan,)), ("p2", (np.inf,))):
        for v in values:
            bad = lib_params(dsrt, M.params(**M.CASES["barrel"][2]))
            setattr(bad, field, v)
            assert call(bad) == -1 and b"dsrt_lens_distort_points" in L.dsrt_last_error(), (field, v)
    assert (out == 7.0).all() and (ok == 9).all()                                               # a refused call writes nothing
    loose = lib_params(dsrt, M.params(**M.CASES["barrel"][2]))
    loose.v1, loose.filter, loose.channels, loose.src_width = np.nan, 9, 0, 0                   # what only the warp reads is not looked at
    assert call(loose) == 0 and L.dsrt_lens_distort_points(C.byref(good), 2, xy.ctypes.data, out.ctypes.data, None) == 0        # ok is optional


# ---- 2. ABI, defaults ----
def test_abi_version_sizes_exports_and_defaults(dsrt):
    capi = dsrt.capi
    assert capi.ABI_VERSION == dsrt.lib.dsrt_abi_version() == 8                                 # additive: the version stays
    with open(os.path.join(ROOT, "include", "dsrt.h")) as f:
        header = f.read()
    listed = [n.strip() for n in re.search(r"purely additive since, version kept: ([^)]*)\)", header).group(1).split(",")]
    for name in NEW_NAMES:
        assert name in listed, name
    for name in FUNCTIONS:
        assert name in capi.EXPORTS and hasattr(dsrt.lib, name)
    assert dsrt.lib.dsrt_sizeof(29) == C.sizeof(capi.DsrtLens) == 92 and dsrt.lib.dsrt_sizeof(30) == C.sizeof(capi.DsrtLensOut) == 24
    assert dsrt.lib.dsrt_sizeof(28) == 0 and dsrt.lib.dsrt_sizeof(31) == 0
    assert re.search(r"#define\s+DSRT_SIZEOF_LENS\s+29\b", header) and re.search(r"#define\s+DSRT_SIZEOF_LENS_OUT\s+30\b", header)
    assert "LENS MODEL" in header and "0x1p-6f" in header and "EXACTLY 12 times" in header
    assert M.ITERATIONS == 12 and float(M.CERTIFICATE) == 2.0 ** -6
    assert (capi.LENS_NEAREST, capi.LENS_BILINEAR, capi.LENS_CUBIC) == (M.NEAREST, M.BILINEAR, M.CUBIC)
    assert (capi.LENS_INVERTED, capi.LENS_ANY_TAP, capi.LENS_ALL_TAPS) == (M.INVERTED, M.ANY_TAP, M.ALL_TAPS)
    d = dsrt.lens_defaults()
    assert {k: getattr(d, k) for k, _ in capi.DsrtLens._fields_} == M.DEFAULTS                  # all coefficients 0, filter 2, channels 3, clamp on
    dsrt.lib.dsrt_lens_defaults(None)                                                           # tolerated
    with pytest.raises(ValueError):
        dsrt.lens_defaults(k4=1.0)


# ---- 3. every refusal of the warp: the context is checked last, so without one every other check runs ----
def test_lens_apply_refusals_without_a_device(dsrt):
    capi, L = dsrt.capi, dsrt.lib
    W, H, kw = M.CASES["barrel"]
    p0 = M.params(**kw)
    n_src = p0["src_width"] * p0["src_height"] * 3
    src = np.zeros(n_src + 1, F)
    image, xy, status = np.full(W * H * 3 + 1, 7.0, F), np.full(W * H * 2, 7.0, F), np.full(W * H, 7, np.uint8)

    def call(desc=None, s=src.ctypes.data, params=None, out=None, host=False, **fields):
        desc = dsrt.make_desc(W, H, 1) if desc is None else desc
        params = lib_params(dsrt, p0) if params is None else params
        for k, v in fields.items():
            setattr(params, k, v)
        out = capi.DsrtLensOut(image.ctypes.data, xy.ctypes.data, status.ctypes.data) if out is None else out
        ref = lambda x: C.byref(x) if x is not False else None                                  # noqa: E731
        head = (None, ref(desc), s, ref(params), ref(out))
        rc = L.dsrt_lens_apply_to_host(*head) if host else L.dsrt_lens_apply(*head, None)
        return rc, L.dsrt_last_error().decode()

    for host in (False, True):
        def refused(words, **kw2):
            rc, why = call(host=host, **kw2)
            assert rc == -1 and words in why and ("dsrt_lens_apply_to_host" if host else "dsrt_lens_apply:") in why, (kw2, why)
        refused("null context")                                                                 # a good call gets as far as the context
        refused("null argument", desc=False)
        refused("null argument", s=None)
        refused("null argument", params=False)
        refused("null argument", out=False)
        for w, h in ((1, 8), (8, 1), (0, 0), (-3, 8), (65536, 32768)):
            refused("width and height" if w < 2 or h < 2 else "2^31", desc=dsrt.make_desc(w, h, 1))
        for w, h in ((1, 8), (8, 1), (0, 4), (8, -1)):
            refused("src_width and src_height", src_width=w, src_height=h)
        refused("2^31", src_width=65536, src_height=32768)
        for f in ("fx", "fy", "src_fx", "src_fy"):
            for v in (0.0, -30.0, np.nan, np.inf):
                refused("must be > 0", **{f: v})
        for f in ("cx", "cy", "src_cx", "src_cy"):
            for v in (np.nan, np.inf, -np.inf):
                refused("principal point", **{f: v})
        for f in ("k1", "k2", "k3", "p1", "p2"):
            for v in (np.nan, np.inf):
                refused("distortion coefficient", **{f: v})
        for f in ("v1", "v2", "v3"):
            for v in (np.nan, -np.inf):
                refused("vignetting coefficient", **{f: v})
        for v in (-1, 3):
            refused("filter", filter=v)
        for v in (0, 5, -1):
            refused("channels", channels=v)
        for v in (-1, 2):
            refused("cos4 and clamp_zero", cos4=v)
            refused("cos4 and clamp_zero", clamp_zero=v)
        refused("no output", out=capi.DsrtLensOut(None, None, None))
        refused("aligned", s=src.ctypes.data + 2)
        refused("aligned", out=capi.DsrtLensOut(image.ctypes.data + 1, None, None))
        refused("aligned", out=capi.DsrtLensOut(None, xy.ctypes.data + 2, None))
        refused("overlaps the source", out=capi.DsrtLensOut(src.ctypes.data + 4 * (n_src - 1), None, None))
        refused("overlaps the source", out=capi.DsrtLensOut(None, None, src.ctypes.data + 5))
        refused("two output ranges overlap", out=capi.DsrtLensOut(image.ctypes.data, image.ctypes.data + 4 * (W * H * 3 - 1), None))
        refused("two output ranges overlap", out=capi.DsrtLensOut(None, xy.ctypes.data, xy.ctypes.data + 8 * W * H - 1))
        refused("null context", out=capi.DsrtLensOut(image.ctypes.data + 4, None, None))         # one word along, still apart from the rest
        refused("null context", out=capi.DsrtLensOut(None, None, status.ctypes.data))            # any one output will do
    assert (image == 7.0).all() and (xy == 7.0).all() and (status == 7).all() and not src.any()  # a refused call touches no buffer


# ---- 4. the model's own invariants ----
def test_zero_coefficients_and_equal_intrinsics_return_the_source():
    """With a power-of-two focal length (((float)x - cx) / fx) * fx + cx == x exactly, so sx, sy are the pixel grid; every filter's weight at t = 0 is 1 on the
    texel itself and +-0 elsewhere, the sum starts at +0.0f, so a finite source comes back bit for bit -- but for -0.0f, which filters 1 and 2 return as +0.0f
    (+0 + -0 = +0); nearest copies words, -0.0f and NaN payloads included.  clamp_zero is off: the source has negative values."""
    rng = np.random.default_rng(4)
    W, H = 23, 11
    for C_ in (1, 3, 4):
        src = rng.standard_normal((H, W, C_)).astype(F)
        src[2, 3], src[5, 7, 0] = F(-0.0), F(0.0)
        for flt in (M.NEAREST, M.BILINEAR, M.CUBIC):
            p = M.params(filter=flt, channels=C_, clamp_zero=0, fill_bits=0xDEADBEEF, **M.centred(W, H, W, H, 32.0))
            s = src.copy()
            if flt == M.NEAREST:
                s.view(np.uint32)[1, 1] = 0x7FC12345                                            # a NaN with a payload: words are copied
            out = M.apply(p, s, W, H)
            ys, xs = np.mgrid[0:H, 0:W]
            assert np.array_equal(out["src_xy"], np.stack([xs, ys], axis=-1).astype(F))
            want_status = np.full((H, W), 7, np.uint8)
            if flt == M.BILINEAR:
                want_status[-1, :], want_status[:, -1] = 3, 3                                   # the 2 x 2 at floorf(s) leaves the frame on the last row and column
            if flt == M.CUBIC:
                want_status[:] = 3
                want_status[1:-2, 1:-2] = 7                                                     # the 4 x 4 at floorf(s) - 1
            assert np.array_equal(out["status"], want_status), (C_, flt)
            want = s if flt == M.NEAREST else np.where(s == 0, F(0.0), s)
            assert np.array_equal(bits(out["image"].reshape(H, W, C_)), bits(want)), (C_, flt)


def test_round_trip_through_the_forward_model(dsrt):
    """For every pixel (x, y) the model flags inverted, dsrt_lens_distort_points(src_xy) comes back to (x, y) within the certificate's 2^-6 plus roundings.  With
    e = EPS, per coordinate (x shown), xd = fl(fl(x - cx) / fx), xr = distort32(xu, yu):
      the certificate      fl(fl(xr - xd) * fx) <= 2^-6            =>  |xr - xd| fx <= 2^-6 (1 + 3 e)
      the map              sx = fl(fl(xu sfx) + scx)               =>  |sx - (xu sfx + scx)| <= e (|xu sfx| + |sx|)
      the helper's input   xu' = fl(fl(sx - scx) / sfx)            =>  |xu' - xu| <= d := e (|xu sfx| + |sx|) / sfx + 2.01 e |sx - scx| / sfx
      its distort32        |xr' - xr| <= L (dx + dy) + 2 rho       L: the largest partial derivative of the exact distort (analytic, float64) around the points,
                                                                    rho = 16 e B: distort32's 16 roundings, each on a magnitude below B = (1 + r2 + |rad| + |dx|)(1 + |xu|)
      its output           ox = fl(fl(xr' fx) + cx)                =>  |ox - (xr' fx + cx)| <= e (|xr' fx| + |ox|)
      the normalisation    |xd fx - (x - cx)| <= 2.01 e |x - cx|
    so |ox - x| <= 2^-6 (1 + 3 e) + fx (L (dx + dy) + 2 rho) + e (2.01 |x - cx| + |xr' fx| + |ox|).  Everything after the first term is below 2e-3 here (the wide case, fx = 60, has the most)."""
    for name in ("barrel", "pincushion", "mixed", "wide"):
        W, H, kw = M.CASES[name]
        p = M.params(**kw)
        xu, yu, inv, sx, sy, _ = M.positions(p, W, H)
        assert inv.mean() > 0.5
        out, ok = dsrt.lens_distort_points(lib_params(dsrt, p), np.stack([sx, sy], axis=-1)[inv])
        assert ok.all()
        ys, xs = np.mgrid[0:H, 0:W]
        q = {k: np.float64(v) for k, v in p.items()}
        xu, yu, sx, sy = (a[inv].astype(np.float64) for a in (xu, yu, sx, sy))
        r2 = xu * xu + yu * yu
        rad = 1 + r2 * (q["k1"] + r2 * (q["k2"] + r2 * q["k3"]))
        drad = q["k1"] + 2 * q["k2"] * r2 + 3 * q["k3"] * r2 * r2                                # d rad / d r2
        tang = 6 * (abs(q["p1"]) + abs(q["p2"])) * (np.abs(xu) + np.abs(yu))                      # bounds every partial derivative of dx and dy
        L = 1.01 * (np.abs(rad) + 2 * r2 * np.abs(drad) + tang).max()                            # |d(xu rad)/dxu| <= |rad| + 2 xu^2 |drad|, the cross terms 2 |xu yu| |drad|
        for axis, (pix, c, f, sf, sc, u, s) in enumerate(((xs[inv], q["cx"], q["fx"], q["src_fx"], q["src_cx"], xu, sx), (ys[inv], q["cy"], q["fy"], q["src_fy"], q["src_cy"], yu, sy))):
            d_x = EPS * (np.abs(xu * q["src_fx"]) + np.abs(sx)) / q["src_fx"] + 2.01 * EPS * np.abs(sx - q["src_cx"]) / q["src_fx"]
            d_y = EPS * (np.abs(yu * q["src_fy"]) + np.abs(sy)) / q["src_fy"] + 2.01 * EPS * np.abs(sy - q["src_cy"]) / q["src_fy"]
            B = (1 + r2 + np.abs(rad) + tang) * (1 + np.abs(u))
            o = out[:, axis].astype(np.float64)
            margin = 2.0 ** -6 * (1 + 3 * EPS) + f * (L * (d_x + d_y) + 2 * 16 * EPS * B) + EPS * (2.01 * np.abs(pix - c) + np.abs(o - c) + np.abs(o))
            assert (margin - 2.0 ** -6).max() < 2e-3
            err = np.abs(o - pix)
            assert (err <= margin).all(), (name, axis, err.max())


def test_the_model_against_float64_on_the_barrel_set():
    """The float32 model against the same formulas and the same twelve steps in float64 (M.reference64), on the barrel set: the source position agrees to a
    tolerance that follows from the operation count.  One step of one coordinate is 17 roundings (xx, yy, xy, r2; six for rad; five for dx or dy; the
    subtraction; the division), each at most EPS times a magnitude below B = (1 + r2 + |rad| + |dx| + |dy|)(1 + |xu| + |yu|), and what follows a rounding divides
    by rad at most once: a step adds at most e_step = 17 EPS B / min(1, rad_min).  The difference of the two sequences obeys e' <= q e + e_step with q the largest
    infinity norm of the step's Jacobian over all pixels and all twelve iterates (finite differences, float64), so it stays below e_step / (1 - q); the start
    xd = fl(fl(x - cx) / fx) is off by 2.01 EPS |xd| and enters every step through (xd - dx) / rad: another 2.01 EPS |xd| / rad_min / (1 - q).  Then
    sx = fl(fl(xu sfx) + scx) adds EPS (|xu sfx| + |sx|).  MEASURED on the CPU: 5.2e-6 pixels in x, 2.1e-6 in y (1.4 ulp of sx); the bound evaluates to 2.9e-4
    pixels (q = 0.34, B = 5.3): the worst case of 17 roundings per step against the handful of ulps that random signs leave."""
    W, H, kw = M.CASES["barrel"]
    p = M.params(**kw)
    xu, yu, inv, sx, sy, _ = M.positions(p, W, H)
    assert inv.all()
    xu64, yu64, sx64, sy64 = M.reference64(p, W, H)
    q_ = {k: np.float64(v) for k, v in p.items()}

    def step(xd, yd, a, b):
        r2 = a * a + b * b
        rad = 1 + r2 * (q_["k1"] + r2 * (q_["k2"] + r2 * q_["k3"]))
        dx = 2 * q_["p1"] * a * b + q_["p2"] * (r2 + 2 * a * a)
        dy = q_["p1"] * (r2 + 2 * b * b) + 2 * q_["p2"] * a * b
        return (xd - dx) / rad, (yd - dy) / rad, r2, rad, dx, dy

    ys, xs = np.mgrid[0:H, 0:W]
    xd, yd = (xs - q_["cx"]) / q_["fx"], (ys - q_["cy"]) / q_["fy"]
    a, b, q, B, rad_min, h = xd, yd, 0.0, 0.0, 1.0, 1e-6
    for _ in range(M.ITERATIONS):
        gx, gy, r2, rad, dx, dy = step(xd, yd, a, b)
        gxa, gya = step(xd, yd, a + h, b)[:2]
        gxb, gyb = step(xd, yd, a, b + h)[:2]
        q = max(q, ((np.abs(gxa - gx) + np.abs(gxb - gx)) / h).max(), ((np.abs(gya - gy) + np.abs(gyb - gy)) / h).max())
        B = max(B, ((1 + r2 + np.abs(rad) + np.abs(dx) + np.abs(dy)) * (1 + np.abs(a) + np.abs(b))).max())
        rad_min = min(rad_min, rad.min())
        a, b = gx, gy
    assert 0.3 < q < 0.7 and rad_min > 0.8, (q, rad_min)
    e_iter = (17 * EPS * B / rad_min + 2.01 * EPS * max(np.abs(xd).max(), np.abs(yd).max()) / rad_min) / (1 - q)
    for s32, s64, u64, sf in ((sx, sx64, xu64, q_["src_fx"]), (sy, sy64, yu64, q_["src_fy"])):
        tol = sf * e_iter + EPS * (np.abs(u64 * sf) + np.abs(s64)).max()
        err = np.abs(s32.astype(np.float64) - s64).max()
        print(f"model against float64: {err:.3g} pixels, bound {tol:.3g} (q = {q:.3f}, B = {B:.3g})")
        assert 1e-4 < tol < 5e-4 and err <= tol, (err, tol)
    # the two agree on the certificate as well: every pixel's float64 residual is far below 2^-6
    r2 = xu64 * xu64 + yu64 * yu64
    rad = 1 + r2 * (q_["k1"] + r2 * (q_["k2"] + r2 * q_["k3"]))
    back = xu64 * rad + 2 * q_["p1"] * xu64 * yu64 + q_["p2"] * (r2 + 2 * xu64 * xu64)
    assert (np.abs(back - xd) * q_["fx"]).max() < 1e-3


def test_the_mixed_case_holds_every_class():
    """The strong barrel folds over inside the frame: every class of pixel -- no preimage, all taps inside, some, none -- holds at least 5 % under Catmull-Rom, so
    that no branch of the kernel passes tests/test_gpu_lens.py vacuously."""
    W, H, kw = M.CASES["mixed"]
    p = M.params(filter=M.CUBIC, channels=1, **kw)
    st = M.apply(p, np.ones((p["src_height"], p["src_width"], 1), F), W, H)["status"]
    shares = {"not inverted": (st == 0).mean(), "all taps inside": (st == 7).mean(), "partly inside": (st == 3).mean(), "wholly outside": (st == 1).mean()}
    assert abs(sum(shares.values()) - 1) < 1e-12 and min(shares.values()) >= 0.05, shares


# ---- 5. the library's own pinhole ----
def test_intrinsics_from_camera_put_the_pixel_centre_rays_on_integer_pixels(dsrt):
    """The pixel-centre directions of the renderer's camera (tests/_temporal_model.pixel_rays: u = (x + 0.5) / (W - 1), rows flipped), taken to normalised
    coordinates xu = -a / cc, yu = b / cc (a, b, cc = D . u, D . v, D . w as in _stars_model.project), land on (x, row) under the returned fx, fy, cx, cy."""
    W, H = 37, 21
    cam = dsrt.camera_look_at((25.0, 18.0, 70.0), (1.0, -2.0, 0.5), 40.0, W, H, 4, 8)
    fx, fy, cx, cy = dsrt.lens_intrinsics_from_camera(cam, W, H)
    _, d = pixel_rays(cam, W, H)
    vec = lambda v: np.array([v.x, v.y, v.z], np.float64)                                       # noqa: E731
    a, b, cc = d @ vec(cam.u), d @ vec(cam.v), d @ vec(cam.w)
    rows, xs = np.mgrid[0:H, 0:W]
    assert (cc < 0).all() and fx > 0 and fy > 0
    assert np.abs(-a / cc * fx + cx - xs).max() < 1e-4 and np.abs(b / cc * fy + cy - rows).max() < 1e-4
    assert abs(cx - (W - 1) / 2) > 0.4 and abs(cy - (H - 1) / 2) > 0.4                          # NOT the frame's centre: the half-pixel of u = (x + 0.5) / (W - 1)
    import _stars_model as S
    fxs, fys, ok = S.project(d.reshape(-1, 3).astype(F), cam, W, H)                             # and the star field's projection agrees
    assert ok.all() and np.abs(fxs - xs.reshape(-1)).max() < 1e-3 and np.abs(fys - rows.reshape(-1)).max() < 1e-3
    out = np.full(4, 7.0, F)
    L = dsrt.lib
    assert L.dsrt_lens_intrinsics_from_camera(None, W, H, out.ctypes.data) == -1 and L.dsrt_lens_intrinsics_from_camera(C.byref(cam), W, H, None) == -1
    assert L.dsrt_lens_intrinsics_from_camera(C.byref(cam), 1, H, out.ctypes.data) == -1 and L.dsrt_lens_intrinsics_from_camera(C.byref(cam), W, 0, out.ctypes.data) == -1
    flat = dsrt.capi.GPUCamera()
    assert L.dsrt_lens_intrinsics_from_camera(C.byref(flat), W, H, out.ctypes.data) == -1 and (out == 7.0).all()


# ---- 6. the CLI refuses a malformed --lens before it needs a device ----
def _cli(tmp_path, spec, *flags, rng_mode=("--rng-mode", "1")):
    return subprocess.run([EXE, "--obj", "no_such_mesh.obj", *rng_mode, "--spp", "4", "--output_dir", str(tmp_path / "out"), "--lens", spec, *flags],
                          capture_output=True, text=True, timeout=60)


def test_cli_refuses_a_bad_lens_spec(dsrt, tmp_path):
    for spec in ("", ",k1=0.1", "k1", "k1=", "k1=abc", "k1=nan", "k2=inf", "k1=1e60", "k4=0.1", "zoom=0", "zoom=-2", "zoom=nan", "vig=0.1", "vig=0.1:0.2", "vig=a:b:c",
                 "vig=0.1:0.2:nan", "cos4=2", "filter=", "filter=lanczos", "filter", "k1=-0.2,", "k1=-0.2,,k2=0.1"):
        r = _cli(tmp_path, spec)
        assert r.returncode == 2 and "--lens" in r.stderr, (spec, r.returncode, r.stderr)
        assert not (tmp_path / "out").exists()
    for spec in ("k1=-0.25", "k1=-0.25,k2=0.05,k3=0,p1=0.002,p2=-0.001,zoom=1.1,vig=-0.3:0.05:0,cos4,filter=linear", "filter=nearest,cos4=0", "zoom=2"):
        r = _cli(tmp_path, spec)                                                                # past the spec: it is the mesh that is missing
        assert r.returncode != 0 and "--lens" not in r.stderr, (spec, r.stderr)


def test_cli_refuses_what_sensor_refuses_and_ignores_lens_in_rng_mode_0(dsrt, tmp_path):
    for flags in (("--adaptive", "0.1"), ("--passes", "2"), ("--gbuffer",), ("--spp", "1")):
        r = _cli(tmp_path, "k1=-0.2", *flags)
        assert r.returncode == 2 and "--lens" in r.stderr, (flags, r.stderr)
    r = _cli(tmp_path, "k1=-0.2", rng_mode=())
    assert r.returncode != 0 and r.returncode != 2 and "--lens needs --rng-mode 1 (or --fast): ignored" in r.stderr
