"""The star field's specification (include/dsrt.h, POINT SOURCES) where it does not depend on the kernels: the numpy model of tests/_stars_model.py -- the
uint64 -> float32 conversion it relies on, order independence, the round-to-even ties, flux conservation, the projection against the pixel-centre rays -- and
the host half of the library: ABI, the catalogue helpers, the refusals that need no device, and the CLI's usage errors.  No GPU."""
import ctypes as C
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from conftest import ROOT
import _stars_model as M
from _stars_model import F
from _temporal_model import exact_camera, pixel_rays

NEW_NAMES = ("DsrtStars", "DsrtStarsOut", "dsrt_render_stars", "dsrt_render_stars_to_host", "dsrt_stars_from_catalog", "dsrt_stars_synthetic_catalog",
             "DSRT_SIZEOF_STARS", "DSRT_SIZEOF_STARS_OUT")
FUNCTIONS = tuple(n for n in NEW_NAMES if n.startswith("dsrt_"))
EXE = os.path.join(ROOT, "deep-space-ray-tracer_amd", "dsrt_render")


def exact_dirs(px, py, W, H):
    """Directions that the exact camera projects to (fx, fy) = (px, py) exactly, for W - 1 and H - 1 powers of two and px, py multiples of 1/8:
    s = (px + 0.5) / (W - 1), t = ((H - 1) - py + 0.5) / (H - 1), D = (2 s - 1, 2 t - 1, -1), every operation exact."""
    px, py = np.asarray(px, np.float64), np.asarray(py, np.float64)
    s, t = (px + 0.5) / (W - 1), ((H - 1) - py + 0.5) / (H - 1)
    D = np.stack([2 * s - 1, 2 * t - 1, -np.ones_like(s)], axis=-1)
    assert np.array_equal(D.astype(F).astype(np.float64), D)
    return D.astype(F)


# ---- 1. the conversion the model relies on ----
def test_u64_to_f32_rounds_to_nearest_even_in_one_step():
    rng = np.random.default_rng(11)
    cases = [0, 1, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 2 ** 24 + 2, 2 ** 24 + 3, 2 ** 25 + 2, 2 ** 25 + 6, 2 ** 62 - 1, 2 ** 64 - 1, 2 ** 64 - 2 ** 39, 2 ** 64 - 2 ** 39 - 1]
    for e in (61, 63):                                                      # ties, and one either side of them, where one ulp is 2^(e-23)
        half = 1 << (e - 24)
        for m in (0, 1, 2, 3, (1 << 23) - 1):
            base = (1 << e) + m * 2 * half
            cases += [base + half - 1, base + half, base + half + 1]
    cases += [int(x) for x in rng.integers(0, 2 ** 63, 2000, dtype=np.uint64)]
    cases += [int(x) >> int(s) for x, s in zip(rng.integers(0, 2 ** 63, 2000, dtype=np.uint64), rng.integers(0, 63, 2000))]
    # double rounding would show here: a value just above a tie whose float64 image IS the tie
    cases += [(1 << 61) + (1 << 37) + 1, (1 << 63) + (1 << 39) + 1, (1 << 61) + 3 * (1 << 37) - 1]
    cases = [c for c in cases if c < 2 ** 64]
    got = M.u64_to_f32(np.array(cases, np.uint64))
    want = np.array([M.u64_to_f32_by_integers(c) for c in cases], F)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    for c, w in zip(cases, want):                                           # and the integer rounding itself: nearest, and even on a tie
        w_int = int(Fraction(float(w)))
        ulp = 1 if c < 2 ** 24 else 1 << (c.bit_length() - 24)
        assert abs(w_int - c) * 2 <= ulp, c
        if abs(w_int - c) * 2 == ulp:
            assert (w_int // ulp) % 2 == 0 or w_int == 1 << w_int.bit_length() - 1, c
    assert float(M.u64_to_f32(np.array([2 ** 25 + 2], np.uint64))[0]) == 2.0 ** 25 and float(M.u64_to_f32(np.array([2 ** 25 + 6], np.uint64))[0]) == 2.0 ** 25 + 8


# ---- 2. the model's own invariants ----
def _random_catalogue(rng, n, W, H):
    """Directions around the exact camera's field of view and beyond, fluxes over twelve decades with negative, NaN, tiny and huge ones among them."""
    D = np.stack([rng.uniform(-1.4, 1.4, n), rng.uniform(-1.4, 1.4, n), -np.ones(n)], axis=1)
    D[rng.random(n) < 0.1, 2] = 1.0                                          # behind the camera
    D *= rng.uniform(0.1, 10.0, (n, 1))                                      # need not be unit vectors
    flux = (10.0 ** rng.uniform(-9, 3, (n, 3))).astype(F)
    special = rng.random(n)
    flux[special < 0.05] *= -1
    flux[(special >= 0.05) & (special < 0.08), 1] = np.nan
    flux[(special >= 0.08) & (special < 0.11)] = F(1e30)
    return D.astype(F), flux


def test_a_permuted_catalogue_gives_the_same_bytes():
    rng = np.random.default_rng(3)
    W, H, n = 17, 9, 3000
    D, flux = _random_catalogue(rng, n, W, H)
    lin = rng.random((H, W, 3)).astype(F)
    blocked = rng.random(n) < 0.3
    a = M.render(D, flux, exact_camera(), W, H, blocked, lin)
    perm = rng.permutation(n)
    b = M.render(D[perm], flux[perm], exact_camera(), W, H, blocked[perm], lin)
    assert np.array_equal(a["A"], b["A"]) and np.array_equal(a["layer"].view(np.uint32), b["layer"].view(np.uint32))
    assert np.array_equal(a["linear_out"].view(np.uint32), b["linear_out"].view(np.uint32))
    assert np.array_equal(a["xy"][perm].view(np.uint32), b["xy"].view(np.uint32)) and np.array_equal(a["status"][perm], b["status"])
    st = a["status"]
    for name, mask in (("not projected", st == 0), ("occluded", (st & 3) == 1), ("visible", (st & 2) != 0), ("clipped", (st & 5) == 1)):
        assert mask.mean() > 0.02, name
    assert (a["A"] > 0).any() and int(a["A"].max()) < 2 ** 62
    assert not a["xy"][st == 0].any() and not (st[(st & 1) == 0]).any()


def test_ties_round_to_even_in_the_layer():
    """4096 stars on one pixel centre of the exact camera (all of the flux in the first tap): 2^24 quanta and 1, 3 and 4095 single quanta on top."""
    W, H, n = 9, 5, 4096
    D = np.repeat(exact_dirs([3.0], [2.0], W, H), n, axis=0)
    q = F(2.0 ** -24)
    flux = np.zeros((n, 3), F)
    flux[0] = 1.0
    flux[1, 0] = q
    flux[1:4, 1] = q
    flux[1:, 2] = q
    out = M.render(D, flux, exact_camera(), W, H)
    assert (out["status"] == 7).all() and np.array_equal(out["xy"], np.tile(np.array([3.0, 2.0], F), (n, 1)))
    assert [int(v) for v in out["A"][2, 3]] == [2 ** 24 + 1, 2 ** 24 + 3, 2 ** 24 + 4095]
    assert [float(v) for v in out["layer"][2, 3]] == [1.0, 1.0 + 2.0 ** -22, 1.0 + 4096 * 2.0 ** -24]      # down to even, up to even, up to even
    touched = np.zeros((H, W), bool)
    touched[2, 3] = True
    assert not out["A"][~touched].any()
    lin = np.full((H, W, 3), F(-0.0))
    res = M.render(D, flux, exact_camera(), W, H, linear=lin)["linear_out"]
    assert not np.signbit(res).any()                                        # -0 + (+0) = +0: an untouched pixel comes out as +0


def test_flux_is_conserved_within_the_quantum_and_the_weights_rounding():
    """A star whose four taps are inside deposits its flux f up to: 2^-25 in each of ox and oy (wx and wy are exact: fx - floorf(fx) is), 2^-24 relative in each
    product bq, 2^-24 relative in each flux * bq -- together below 3.01 * 2^-24 * f -- and less than one quantum of 2^-24 lost in each of four truncations."""
    rng = np.random.default_rng(5)
    W, H, n = 17, 9, 400
    cam = exact_camera()
    D = np.stack([rng.uniform(-0.8, 0.8, n), rng.uniform(-0.8, 0.8, n), -np.ones(n)], axis=1).astype(F)
    flux = (10.0 ** rng.uniform(-6, 4, (n, 3))).astype(F)
    fx, fy, ok = M.project(D, cam, W, H)
    for i in range(n):
        A, inside = M.deposits(flux[i:i + 1], fx[i:i + 1], fy[i:i + 1], ok[i:i + 1], W, H)
        assert ok[i] and inside[0]
        for k in range(3):
            total = Fraction(int(A[..., k].sum()), 2 ** 24)
            f = Fraction(float(flux[i, k]))
            assert total <= f * (1 + Fraction(301, 100) / 2 ** 24) and f - total <= f * Fraction(301, 100) / 2 ** 24 + Fraction(4, 2 ** 24), (i, k)


def test_edge_values_in_the_model():
    W, H = 9, 5
    cam = exact_camera()
    inf, nan = np.inf, np.nan
    # the window's borders are excluded; just inside them a star is projected and clipped
    px = np.array([-1.0, -0.875, 8.875, 9.0, 3.0, 3.0, 3.0, 3.0, -0.5, 8.5, -0.5, 8.5])
    py = np.array([2.0, 2.0, 2.0, 2.0, -1.0, -0.875, 4.875, 5.0, -0.5, -0.5, 4.5, 4.5])
    out = M.render(exact_dirs(px, py, W, H), np.ones((12, 3), F), cam, W, H)
    assert list(out["status"]) == [0, 3, 3, 0, 0, 3, 3, 0, 3, 3, 3, 3]
    assert np.array_equal(out["xy"][1], np.array([-0.875, 2.0], F)) and np.array_equal(out["xy"][9], np.array([8.5, -0.5], F))
    for corner, (y, x) in zip((8, 9, 10, 11), ((0, 0), (0, 8), (4, 0), (4, 8))):      # a quarter of the flux lands in the corner pixel, the rest falls off
        one = M.render(exact_dirs(px[corner:corner + 1], py[corner:corner + 1], W, H), np.ones((1, 3), F), cam, W, H)
        assert [int(v) for v in one["A"][y, x]] == [2 ** 22] * 3 and int(one["A"].sum()) == 3 * 2 ** 22
    # D = 0, NaN, +-inf, behind the camera (cc > 0) and in the camera's plane (cc = 0): not projected, by the projection's own tests
    bad = np.array([[0, 0, 0], [nan, 0, -1], [0, nan, -1], [0, 0, nan], [inf, 0, -1], [0, -inf, -1], [0, 0, -inf], [0, 0, inf], [inf, inf, inf], [0.1, 0.1, 1], [1, 0, 0],
                    [-0.0, 0.0, -0.0]], F)
    out = M.render(bad, np.ones((len(bad), 3), F), cam, W, H)
    assert not out["status"].any() and not out["A"].any() and not out["xy"].view(np.uint32).any()
    # fluxes: negative, NaN, below the quantum, and above the cap of 2^16 per deposit
    D = np.repeat(exact_dirs([3.0], [2.0], W, H), 5, axis=0)
    flux = np.array([[-1, nan, 2.0 ** -25], [1e30, inf, 70000.0], [-inf, -0.0, 0.0], [2.0 ** -24, 2.0 ** -24 * 1.5, 65536.0], [1e-45, 1e-40, 3e38]], F)
    for i, want in enumerate(([0, 0, 0], [2 ** 40] * 3, [0, 0, 0], [1, 1, 2 ** 40], [0, 0, 2 ** 40])):
        assert [int(v) for v in M.render(D[i:i + 1], flux[i:i + 1], cam, W, H)["A"][2, 3]] == want, i


def test_pixel_centre_rays_project_to_their_pixels():
    """The projection inverts the G-buffer's pixel-centre ray: (fx, fy) = (x, row) up to rounding, for a camera of dsrt_camera_look_at's kind (an orthonormal
    u, v, w; horizontal along u, vertical along v; the lower left corner one unit down -w) and directions of any length."""
    W, H = 37, 21
    w = np.array([0.4479, 0.4482, 0.7736])
    w /= np.linalg.norm(w)
    u = np.cross([0.0, 1.0, 0.0], w)
    u /= np.linalg.norm(u)
    v = np.cross(w, u)
    origin = np.array([3.0, 2.0, 9.0])
    cam = {"origin": origin, "horizontal": 2.2 * u, "vertical": 1.3 * v, "lower_left_corner": origin - 1.1 * u - 0.65 * v - w, "u": u, "v": v, "w": w}
    _, d = pixel_rays(cam, W, H)
    fx, fy, ok = M.project((d * 7.5).reshape(-1, 3).astype(F), cam, W, H)
    rows, xs = np.mgrid[0:H, 0:W]
    assert ok.all() and np.abs(fx - xs.reshape(-1)).max() < 1e-3 and np.abs(fy - rows.reshape(-1)).max() < 1e-3


# ---- 3. ABI and helpers ----
def test_abi_version_sizes_and_exports(dsrt):
    capi = dsrt.capi
    assert capi.ABI_VERSION == dsrt.lib.dsrt_abi_version() == 8                         # additive: the version stays
    with open(os.path.join(ROOT, "include", "dsrt.h")) as f:
        header = f.read()
    additive = re.search(r"purely additive since, version kept: ([^)]*)\)", header).group(1)
    listed = [n.strip() for n in additive.split(",")]
    for name in NEW_NAMES:
        assert name in listed, name
    for name in FUNCTIONS:
        assert name in capi.EXPORTS and hasattr(dsrt.lib, name)
    assert dsrt.lib.dsrt_sizeof(26) == C.sizeof(capi.DsrtStars) == 32 and dsrt.lib.dsrt_sizeof(27) == C.sizeof(capi.DsrtStarsOut) == 32
    assert dsrt.lib.dsrt_sizeof(25) == 0 and dsrt.lib.dsrt_sizeof(28) == 0
    assert re.search(r"#define\s+DSRT_SIZEOF_STARS\s+26\b", header) and re.search(r"#define\s+DSRT_SIZEOF_STARS_OUT\s+27\b", header)
    assert "POINT SOURCES" in header and "16777216.0f" in header and "1099511627776.0f" in header and "0x1p-24f" in header
    assert float(M.QUANTA) == 2.0 ** 24 and float(M.CAP) == 2.0 ** 40 and float(M.SCALE) == 2.0 ** -24
    assert (capi.STAR_PROJECTED, capi.STAR_VISIBLE, capi.STAR_INSIDE) == (M.PROJECTED, M.VISIBLE, M.INSIDE) and capi.MAX_STARS == 2 ** 22


def test_stars_from_catalog(dsrt):
    rng = np.random.default_rng(2)
    ra, dec, mag = rng.uniform(0, 360, 500), rng.uniform(-90, 90, 500), rng.uniform(-1.5, 12, 500)
    ra[:4], dec[:4], mag[:4] = (0, 90, 180, 0), (0, 0, 0, 90), (0, 5, 2.5, -2.5)
    dirs, flux = dsrt.stars_from_catalog(ra, dec, mag, (2.0, 1.0, 0.5))
    a, d = np.radians(ra), np.radians(dec)
    want = np.stack([np.cos(d) * np.cos(a), np.cos(d) * np.sin(a), np.sin(d)], axis=1)
    assert dirs.dtype == np.float64 and np.abs(dirs - want).max() < 1e-14 and np.abs(np.linalg.norm(dirs, axis=1) - 1).max() < 1e-14
    assert np.abs(dirs[:4] - np.array([[1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, 0, 1]])).max() < 1e-15
    want_flux = np.array([2.0, 1.0, 0.5]) * (10.0 ** (-0.4 * mag))[:, None]
    assert flux.dtype == F and np.abs(flux / want_flux - 1).max() < 2e-7
    assert np.allclose(flux[:4, 1], [1.0, 0.01, 0.1, 10.0], rtol=2e-7)
    empty = dsrt.stars_from_catalog([], [], [])
    assert empty[0].shape == (0, 3) and empty[1].shape == (0, 3)
    one = np.zeros(1)
    f3 = np.ones(3, F)
    out_d, out_f = np.full(3, 7.0), np.full(3, 7.0, F)
    L = dsrt.lib
    assert L.dsrt_stars_from_catalog(-1, one.ctypes.data, one.ctypes.data, one.ctypes.data, f3.ctypes.data, out_d.ctypes.data, out_f.ctypes.data) == -1
    assert L.dsrt_stars_from_catalog(1, None, one.ctypes.data, one.ctypes.data, f3.ctypes.data, out_d.ctypes.data, out_f.ctypes.data) == -1
    assert L.dsrt_stars_from_catalog(1, one.ctypes.data, one.ctypes.data, one.ctypes.data, None, out_d.ctypes.data, out_f.ctypes.data) == -1
    assert L.dsrt_stars_from_catalog(1, one.ctypes.data, one.ctypes.data, one.ctypes.data, f3.ctypes.data, None, out_f.ctypes.data) == -1
    assert (out_d == 7.0).all() and (out_f == 7.0).all()
    with pytest.raises(ValueError):
        dsrt.stars_from_catalog([1, 2], [1], [1, 2])


def test_synthetic_catalogue(dsrt):
    n = 1 << 16
    ra, dec, mag = dsrt.synthetic_star_catalog(7, n, 1.0, 8.0)
    again = dsrt.synthetic_star_catalog(7, n, 1.0, 8.0)
    other = dsrt.synthetic_star_catalog(8, n, 1.0, 8.0)
    assert all(np.array_equal(x, y) for x, y in zip((ra, dec, mag), again)) and not np.array_equal(ra, other[0])
    assert ra.min() >= 0 and ra.max() < 360 and dec.min() >= -90 and dec.max() <= 90 and mag.min() >= 1.0 and mag.max() <= 8.0
    dirs, _ = dsrt.stars_from_catalog(ra, dec, mag)
    # uniform on the sphere: each coordinate has mean 0 and variance 1/3; five standard errors of the mean, sqrt(1 / (3 n))
    assert np.abs(dirs.mean(axis=0)).max() < 5 * np.sqrt(1 / (3 * n))
    assert np.abs((dirs ** 2).mean(axis=0) - 1 / 3).max() < 5 * np.sqrt(4 / 45 / n)      # var(x^2) = 1/5 - 1/9
    # N(< m) ~ 10^(0.5 m): half of the stars lie above m with 10^(0.5 m) = (10^0.5 + 10^4) / 2
    m_half = 2 * np.log10((10 ** 0.5 + 10 ** 4) / 2)
    assert abs((mag < m_half).mean() - 0.5) < 5 * np.sqrt(0.25 / n)
    assert dsrt.synthetic_star_catalog(1, 0)[0].shape == (0,)
    z = np.full(4, 7.0)
    L = dsrt.lib
    for args in ((1, -1, 0.0, 6.0), (1, 4, 6.0, 0.0), (1, 4, float("nan"), 6.0), (1, 4, 0.0, float("inf"))):
        assert L.dsrt_stars_synthetic_catalog(*args, z.ctypes.data, z.ctypes.data, z.ctypes.data) == -1
    assert L.dsrt_stars_synthetic_catalog(1, 4, 0.0, 6.0, None, z.ctypes.data, z.ctypes.data) == -1
    assert (z == 7.0).all()


def test_refusals_that_need_no_device(dsrt):
    capi = dsrt.capi
    desc = dsrt.make_desc(8, 8, 1)
    buf = np.full(8 * 8 * 3, 7.0, F)
    stars, out = capi.DsrtStars(0, 1, None, None, None), capi.DsrtStarsOut(layer=buf.ctypes.data)
    L = dsrt.lib
    assert L.dsrt_render_stars(None, C.byref(desc), C.byref(stars), C.byref(out), None, None) == -1 and b"null argument" in L.dsrt_last_error()
    assert L.dsrt_render_stars_to_host(None, C.byref(desc), C.byref(stars), C.byref(out), None) == -1 and b"null argument" in L.dsrt_last_error()
    assert (buf == 7.0).all()


# ---- 4. the CLI refuses a malformed --stars before it needs a device ----
def _cli(tmp_path, spec, *flags):
    return subprocess.run([EXE, "--obj", "no_such_mesh.obj", "--rng-mode", "1", "--spp", "4", "--output_dir", str(tmp_path / "out"), "--stars", spec, *flags],
                          capture_output=True, text=True, timeout=60)


def test_cli_refuses_a_bad_stars_spec(dsrt, tmp_path):
    good = tmp_path / "cat.txt"
    good.write_text("# ra dec mag\n10.5 -20.25 3.5\n\n  200 45 1\n")
    for name, text in (("short.txt", "10 20\n"), ("long.txt", "10 20 3 4\n"), ("words.txt", "ten 20 3\n"), ("nan.txt", "10 nan 3\n")):
        (tmp_path / name).write_text(text)
    for spec in ("", ",flux=2", str(tmp_path / "no_such_file.txt"), f"{good},flux=", f"{good},flux=abc", f"{good},flux=-1", f"{good},flux=nan", f"{good},occlusion=2",
                 f"{good},colour=1", f"{good},flux", f"{good},", str(tmp_path / "short.txt"), str(tmp_path / "long.txt"), str(tmp_path / "words.txt"), str(tmp_path / "nan.txt")):
        r = _cli(tmp_path, spec)
        assert r.returncode == 2 and "--stars" in r.stderr, (spec, r.returncode, r.stderr)
        assert not (tmp_path / "out").exists()
    for spec in (str(good), f"{good},flux=2.5", f"{good},occlusion=0,flux=1e3"):         # past the spec: it is the mesh that is missing
        r = _cli(tmp_path, spec)
        assert r.returncode != 0 and "--stars" not in r.stderr, (spec, r.stderr)


def test_cli_refuses_what_sensor_refuses_and_ignores_stars_in_rng_mode_0(dsrt, tmp_path):
    good = tmp_path / "cat.txt"
    good.write_text("10 20 3\n")
    for flags in (("--adaptive", "0.1"), ("--passes", "2"), ("--gbuffer",), ("--spp", "1")):
        r = _cli(tmp_path, str(good), *flags)
        assert r.returncode == 2 and "--stars" in r.stderr, (flags, r.stderr)
    r = subprocess.run([EXE, "--obj", "no_such_mesh.obj", "--output_dir", str(tmp_path / "out0"), "--stars", str(good)], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and r.returncode != 2 and "--stars needs --rng-mode 1 (or --fast): ignored" in r.stderr
