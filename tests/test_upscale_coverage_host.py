"""The upscaler with coverage without a GPU (include/dsrt.h, COVERAGE-AWARE UPSCALER): the two identities and the levels of the numpy model
(tests/_upscale_coverage_model.py), every refusal that needs no device, exports, the CLI's usage errors, and the quality of the result on two parity scenes -- on
the model alone: the kernel equals it bit for bit (tests/test_gpu_upscale_coverage.py), so what the model achieves is what the library achieves."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _coverage_model as CM
from conftest import ASSETS, ROOT
from _denoise_model import DEFAULTS as DENOISE_DEFAULTS, F, denoise, start
from _sample_sets import SetOracle, parity_case
from _upscale_coverage_model import ALPHA_MIN, synthetic_alphas, upscale_coverage
from _upscale_model import DEFAULTS, GB_SUN_VISIBLE, GUIDES, synthetic_pair, synthetic_raster, upscale
from test_denoise_host import synthetic_frame

SEED_A, SEED_B = 0xDEADBEEF00001337, 0x0123456789ABCDEF
CHANNELS = GUIDES + ("flags",)
ALPHA_MINS = (1 / 64, 1 / 16, 1 / 8, 1 / 4)


def _same(got, want, what):
    g, w = (np.asarray(a).view(np.uint32) if np.asarray(a).dtype == np.float32 else np.asarray(a) for a in (got, want))
    assert g.shape == w.shape and (g == w).all(), what


# ---- 1. the two identities ----
@pytest.mark.parametrize("w, h, W, H", [(37, 29, 74, 58), (2, 2, 5, 3)])
def test_alpha_null_and_alpha_one_are_the_plain_upscaler_bit_for_bit(w, h, W, H):
    rng = np.random.default_rng(31 * W + H)
    c, v, lo, hi, _ = synthetic_pair(rng, w, h, W, H)
    ys, xs = np.mgrid[0:H, 0:W]
    odd = (xs % 7 == 3) & (ys % 5 == 2) & (hi["range"] < np.inf)                        # no tap shares these normals: the plain upscaler's level 2
    hi["normal"] = np.where(odd[..., None], np.array([0, 1, 0], F), hi["normal"]).astype(F)
    for flags, with_var in ((True, True), (False, False)):
        lo_m, hi_m = ({k: g[k] for k in (CHANNELS if flags else GUIDES)} for g in (lo, hi))
        want = upscale(c, v if with_var else None, lo_m, hi_m, **DEFAULTS)
        ones = (np.ones((h, w), F), np.ones((H, W), F))
        for alphas, amin in (((None, None), ALPHA_MIN), (ones, ALPHA_MIN), (ones, 1.0), (ones, 1e-6)):
            lin, var, sup, level = upscale_coverage(c, v if with_var else None, lo_m, hi_m, *alphas, alpha_min=amin, **DEFAULTS)
            for got, wnt, name in zip((lin, var, sup), want, ("linear", "var", "support")):
                _same(got, wnt, (name, flags, alphas[0] is None, amin))
            hit = hi["range"] <= np.finfo(F).max
            assert (level[~hit] == 0).all() and ((level == 1) == (sup > 0)).all()
            # what the plain upscaler calls level 2 is level 3 without alphas and, with every tap usable, the new level 2
            assert set(np.unique(level[hit & (sup == 0)])) <= ({3} if alphas[0] is None else {2})
        if W > 5:
            assert (hit & (want[2] == 0)).sum() > 10


# ---- 2. the levels, on hand-built rasters ----
def _plane(w, h, W, H, edge=None):
    """One plane facing the camera, one albedo, every pixel hit (as test_upscale_host._half_lit); sunlit where u < edge (everywhere without one)."""
    def raster(W, H):
        ys, xs = np.mgrid[0:H, 0:W]
        u, v = (xs + 0.5) / (W - 1), ((H - 1 - ys) + 0.5) / (H - 1)
        X = np.stack([(u - 0.5) * 4, (v - 0.5) * 3, np.full_like(u, -10.0)], -1).astype(F)
        sun = u < edge if edge is not None else np.ones_like(u, bool)
        return {"normal": np.broadcast_to(np.array([0, 0, 1], F), X.shape).copy(), "position": X, "albedo": np.full(X.shape, 0.6, F),
                "range": np.sqrt((X.astype(np.float64) ** 2).sum(-1)).astype(F), "flags": np.where(sun, 1 | GB_SUN_VISIBLE, 1).astype(np.uint8)}
    return raster(w, h), raster(W, H)


def test_an_output_pixel_without_coverage_is_level_0_and_exactly_zero():
    w, h, W, H = 20, 12, 40, 24
    lo, hi = _plane(w, h, W, H)
    rng = np.random.default_rng(3)
    c, v = rng.random((h, w, 3)).astype(F), rng.random((h, w, 3)).astype(F)
    a_hi = np.full((H, W), 0.5, F)
    a_hi[3, 4], a_hi[5, 6], a_hi[7, 8], a_hi[9, 10] = 0.0, np.nan, -0.25, -0.0
    hi["range"][11, 12] = np.inf
    hi["range"][13, 14] = np.nan
    lin, var, sup, level = upscale_coverage(c, v, lo, hi, np.full((h, w), 0.5, F), a_hi, **DEFAULTS)
    dead = np.zeros((H, W), bool)
    for yx in ((3, 4), (5, 6), (7, 8), (9, 10), (11, 12), (13, 14)):
        dead[yx] = True
    assert (level[dead] == 0).all() and (level[~dead] == 1).all()
    for a in (lin, var, sup):
        assert not a[dead].view(np.uint32).any()                                     # +0, not -0, not NaN
    assert (sup[~dead] > 0).all() and np.isfinite(lin).all() and np.isfinite(var).all()


def test_a_patch_below_alpha_min_reaches_level_3_and_equals_the_plain_level_2():
    w, h, W, H = 20, 12, 40, 24
    lo, hi = _plane(w, h, W, H)
    rng = np.random.default_rng(4)
    c, v = rng.random((h, w, 3)).astype(F), rng.random((h, w, 3)).astype(F)
    a_lo = np.ones((h, w), F)
    a_lo[2:9, 5:13] = np.nextafter(F(ALPHA_MIN), F(0))                                 # a patch wider than any 4 x 4 footprint, just below the threshold
    a_lo[4, 8] = np.nan
    a_hi = np.full((H, W), 0.75, F)
    lin, var, sup, level = upscale_coverage(c, v, lo, hi, a_lo, a_hi, **DEFAULTS)
    three = level == 3
    assert three.sum() > 20 and set(np.unique(level)) == {1, 3}
    # UPSCALER's level 2 is what the plain model gives where no guided tap counts: a frame whose output normals no tap shares is level 2 throughout
    flat_hi = {**hi, "normal": np.broadcast_to(np.array([0, 1, 0], F), hi["normal"].shape).copy()}
    p_lin, p_var, p_sup = upscale(c, v, lo, flat_hi, **DEFAULTS)
    assert not p_sup.any()
    _same(lin[three], p_lin[three], "level 3 colour: the mixed mean, not multiplied by alpha")
    _same(var[three], p_var[three], "level 3 variance")
    assert not sup[three].any() and ((sup > 0) == (level == 1)).all()


def test_usable_taps_all_across_the_sun_edge_reach_level_2():
    """Output pixels in shadow next to an edge whose shadowed low-resolution side is not usable: level 1 finds only sunlit taps (skipped), level 2 takes them."""
    w, h, W, H = 20, 12, 40, 24
    lo, hi = _plane(w, h, W, H, edge=0.53)
    c = np.where((lo["flags"] & GB_SUN_VISIBLE).astype(bool)[..., None], F(0.8), F(0.1)) * np.ones(3, F)
    sun_lo = (lo["flags"] & GB_SUN_VISIBLE).astype(bool)
    a_lo = np.where(sun_lo, F(0.5), F(0.01)).astype(F)                                  # the shadowed side: below alpha_min
    c = (c * a_lo[..., None]).astype(F)
    a_hi = np.full((H, W), 0.25, F)
    lin, _, sup, level = upscale_coverage(c, None, lo, hi, a_lo, a_hi, **DEFAULTS)
    shadow_hi = ~(hi["flags"] & GB_SUN_VISIBLE).astype(bool)
    two = level == 2
    assert two.sum() > 10 and shadow_hi[two].all()                                   # only shadowed output pixels can lose every guided tap here
    assert not sup[two].any() and ((sup > 0) == (level == 1)).all()
    np.testing.assert_allclose(lin[two], 0.8 * 0.25, rtol=1e-5)                        # the usable taps' covered colour times the pixel's own alpha
    assert (level[shadow_hi & ~two] == 3).all() and (level[~shadow_hi] == 1).all()
    # without the sun bit the same pixels are guided
    _, _, _, free = upscale_coverage(c, None, lo, hi, a_lo, a_hi, **{**DEFAULTS, "use_sun": 0})
    assert (free[two] == 1).all()


def test_a_constant_covered_colour_stays_constant():
    """Inputs alpha_lo * C, output C * aP at levels 1 and 2.  Roundings: the product alpha_lo * C, the quotient by alpha_lo, at most sixteen products and
    additions in each of the two sums, the quotient, the product with aP: 36 roundings of 2^-24 at the most, 2.2e-6; ten times margin."""
    rng = np.random.default_rng(12)
    col = np.array([0.37, 0.052, 0.81], F)
    for (w, h, W, H) in ((37, 29, 100, 77), (37, 29, 74, 58), (20, 12, 20, 12)):
        _, _, lo, hi, _ = synthetic_pair(rng, w, h, W, H)
        a_lo = (0.02 + 0.98 * rng.random((h, w))).astype(F)                              # some below alpha_min: not usable
        a_hi = (1.0 - rng.random((H, W))).astype(F)                                      # (0, 1]
        c = (a_lo[..., None] * col).astype(F)
        lin, _, sup, level = upscale_coverage(c, None, lo, hi, a_lo, a_hi, **DEFAULTS)
        at = (level == 1) | (level == 2)
        assert (level == 1).sum() > 0.5 * (hi["range"] < np.inf).sum()
        assert np.abs(lin[at] / (col * a_hi[at][:, None]) - 1).max() < 2.2e-5
        assert not lin[level == 0].any() and ((sup > 0) == (level == 1)).all()


# ---- 3. finite values and sizes ----
@pytest.mark.parametrize("w, h, W, H", [(2, 2, 2, 2), (2, 2, 5, 3), (37, 29, 100, 77)])
def test_sizes_run_with_no_index_out_of_range_and_small_alphas_stay_finite(w, h, W, H):
    """numpy raises on an index out of range, and the model clips only indices it then masks.  Colours from the denoiser's synthetic frame scaled by their alpha
    (a mean is alpha times a bounded radiance), alphas as small as 1/64 with alpha_min 1/64: nothing becomes inf or NaN."""
    rng = np.random.default_rng(100 * w + W)
    S, S2, n, _, _ = synthetic_frame(rng, w, h, spp=4)
    c, v = start(S, S2, n)
    lo, _ = synthetic_raster(w, h)
    hi, _ = synthetic_raster(W, H)
    a_lo = rng.choice(np.array([1 / 64, 1 / 32, 0.5, 1.0], F), (h, w)).astype(F)
    a_hi = rng.choice(np.array([1 / 64, 0.25, 1.0], F), (H, W)).astype(F)
    c, v = (c * a_lo[..., None]).astype(F), (v * (a_lo * a_lo)[..., None]).astype(F)
    lin, var, sup, level = upscale_coverage(c, v, lo, hi, a_lo, a_hi, alpha_min=1 / 64, **DEFAULTS)
    assert lin.shape == (H, W, 3) and var.shape == (H, W, 3) and sup.shape == (H, W) and level.shape == (H, W) and level.dtype == np.uint8
    assert np.isfinite(lin).all() and np.isfinite(var).all() and np.isfinite(sup).all()
    hit = hi["range"] < np.inf
    assert (level[hit] >= 1).all() and (level[hit] <= 2).all() and (level[~hit] == 0).all()       # every tap is usable: level 3 is not reached
    # the synthetic alphas of the GPU tests (0, NaN, the threshold's neighbours) on the same sizes
    s_lo, s_hi = synthetic_alphas(rng, lo, hi)
    lin, var, sup, level = upscale_coverage(c, v, lo, hi, s_lo, s_hi, **DEFAULTS)
    assert np.isfinite(lin).all() and np.isfinite(var).all() and np.isfinite(sup).all() and ((sup > 0) == (level == 1)).all()
    if W > 5:
        assert {0, 1, 3} <= set(np.unique(level))


# ---- 4. ABI, refusals, CLI ----
NEW = ("dsrt_upscale_coverage_alpha_min", "dsrt_upscale_guided_coverage", "dsrt_upscale_guided_coverage_to_host", "dsrt_render_upscaled_coverage_to_host")


def test_exports_version_and_methods(dsrt):
    capi = dsrt.capi
    assert capi.ABI_VERSION == dsrt.lib.dsrt_abi_version() == capi.header_abi_version() == 8          # additive: the version stays
    for name in NEW:
        assert name in capi.EXPORTS and hasattr(dsrt.lib, name)
    for m in ("upscale_guided_coverage", "upscale_guided_coverage_to_host", "render_upscaled_coverage_to_host"):
        assert hasattr(dsrt.Context, m)
    assert F(dsrt.upscale_coverage_alpha_min()) == F(dsrt.lib.dsrt_upscale_coverage_alpha_min()) == F(ALPHA_MIN) == F(0.125)
    assert dsrt.lib.dsrt_sizeof(15) == C.sizeof(capi.DsrtUpscaleGuides) and dsrt.lib.dsrt_sizeof(16) == C.sizeof(capi.DsrtUpscale)      # no struct changed


def test_refusals_that_need_no_device(dsrt):
    """Every argument check comes before the context or any buffer is looked at: a stand-in for the context and host arrays do.  Every buffer is filled with a
    sentinel and must still hold it afterwards."""
    capi, lib = dsrt.capi, dsrt.lib
    w, h, W, H = 6, 4, 12, 8
    ctx = C.cast(C.create_string_buffer(64), C.c_void_p)                            # never dereferenced: every call below is refused
    f32 = lambda n, k: np.full(n * k + 1, -7.5, np.float32)                          # noqa: E731
    lo = dict(lin=f32(w * h, 3), var=f32(w * h, 3), N=f32(w * h, 3), X=f32(w * h, 3), A=f32(w * h, 3), R=f32(w * h, 1), fl=np.full(w * h, 0x5A, np.uint8))
    hi = dict(N=f32(W * H, 3), X=f32(W * H, 3), A=f32(W * H, 3), R=f32(W * H, 1), fl=np.full(W * H, 0x5A, np.uint8))
    a_lo, a_hi = f32(w * h, 1), f32(W * H, 1)
    rgb, o32, lin, var, sup, lev = np.full(W * H * 3, 0x5A, np.uint8), f32(W * H, 3), f32(W * H, 3), f32(W * H, 3), f32(W * H, 1), np.full(W * H, 0x5A, np.uint8)
    everything = list(lo.values()) + list(hi.values()) + [a_lo, a_hi, rgb, o32, lin, var, sup, lev]
    ptr = lambda a, off=0: C.c_void_p(a.ctypes.data + off) if a is not None else None   # noqa: E731
    good = dsrt.make_desc(W, H, 4, rng_mode=1)
    G = lambda g: (g["N"], g["X"], g["A"], g["R"], g["fl"])                          # noqa: E731

    def call(ctx=ctx, desc=good, size=(w, h), c=lo["lin"], v=lo["var"], lo_g=G(lo), hi_g=G(hi), alphas=(a_lo, a_hi), amin=0.0625, params="default",
             outs=(rgb, None, lin, var, sup, lev), off=(0,) * 6, fn="dev"):
        gl = capi.DsrtUpscaleGuides(*[ptr(x) for x in lo_g]) if lo_g is not None else None
        gh = capi.DsrtUpscaleGuides(*[ptr(x) for x in hi_g]) if hi_g is not None else None
        p = dsrt.upscale_defaults() if params == "default" else params
        ref = lambda x: C.byref(x) if x is not None else None                       # noqa: E731
        args = [ctx, ref(desc), size[0], size[1], ptr(c), ptr(v), ref(gl), ref(gh), ptr(alphas[0]), ptr(alphas[1]), C.c_float(amin), ref(p)] + [ptr(o, k) for o, k in zip(outs, off)]
        return lib.dsrt_upscale_guided_coverage(*args, None) if fn == "dev" else lib.dsrt_upscale_guided_coverage_to_host(*args)

    P = lambda **kw: dsrt.upscale_defaults(**kw)                                     # noqa: E731
    without = lambda g, k: tuple(None if i == k else x for i, x in enumerate(G(g)))  # noqa: E731
    nan = float("nan")
    cases = {
        # what dsrt_upscale_guided refuses
        "NULL ctx": call(ctx=None), "NULL desc": call(desc=None), "NULL colour": call(c=None), "NULL lo guides": call(lo_g=None), "NULL hi guides": call(hi_g=None),
        "NULL params": call(params=None),
        **{f"NULL lo channel {k}": call(lo_g=without(lo, k)) for k in range(4)}, **{f"NULL hi channel {k}": call(hi_g=without(hi, k)) for k in range(4)},
        "rng_mode 0": call(desc=dsrt.make_desc(W, H, 4, rng_mode=0)), "shards": call(desc=dsrt.make_desc(W, H, 4, rng_mode=1, shard_count=2)),
        "math_mode 2": call(desc=dsrt.make_desc(W, H, 4, rng_mode=1, math_mode=2)),
        "lo_width 1": call(size=(1, h)), "lo_height negative": call(size=(w, -3)), "W < lo_width": call(size=(W + 1, h)), "H < lo_height": call(size=(w, H + 1)),
        "normal_power_log2 9": call(params=P(normal_power_log2=9)), "sigma_z 0": call(params=P(sigma_z=0.0)), "sigma_a NaN": call(params=P(sigma_a=nan)),
        "no output": call(outs=(None,) * 6), "var without lo var": call(v=None),
        "misaligned colour": call(c=lo["lin"].view(np.uint8)[2:]), "misaligned hi guide": call(hi_g=(hi["N"], hi["X"], hi["A"], hi["R"].view(np.uint8)[2:], hi["fl"])),
        "misaligned linear": call(off=(0, 0, 2, 0, 0, 0)), "output over a hi input": call(outs=(rgb, None, hi["N"], var, sup, lev)),
        "two outputs overlap": call(outs=(rgb, None, lin, lin, sup, lev)),
        # its own
        "only the lo alpha": call(alphas=(a_lo, None)), "only the hi alpha": call(alphas=(None, a_hi)),
        "alpha_min 0": call(amin=0.0), "alpha_min negative": call(amin=-0.5), "alpha_min above 1": call(amin=1.0000001), "alpha_min NaN": call(amin=nan),
        "alpha_min NaN without alphas": call(alphas=(None, None), amin=nan, outs=(rgb, None, lin, var, sup, None)),
        "level without alphas": call(alphas=(None, None)),
        "misaligned lo alpha": call(alphas=(a_lo.view(np.uint8)[2:], a_hi)), "misaligned hi alpha": call(alphas=(a_lo, a_hi.view(np.uint8)[1:])),
        "level over an output": call(outs=(rgb, None, lin, var, sup, rgb)), "level over an input": call(outs=(rgb, None, lin, var, sup, hi["fl"])),
        "level over the lo alpha": call(outs=(rgb, None, lin, var, sup, a_lo.view(np.uint8))),
        "lo alpha over an output": call(alphas=(lin, a_hi)), "hi alpha over an output": call(alphas=(a_lo, sup)), "hi alpha over the level": call(alphas=(a_lo, lev.view(np.uint8)[:W * H // 4 * 4].view(np.float32))),
        "host form: NULL ctx": call(ctx=None, fn="host"), "host form: one alpha": call(alphas=(a_lo, None), fn="host"), "host form: alpha_min NaN": call(amin=nan, fn="host"),
        "host form: no output": call(outs=(None,) * 6, fn="host"), "host form: level over an output": call(outs=(rgb, None, lin, var, sup, rgb), fn="host"),
    }
    assert {k: v for k, v in cases.items() if v != -1} == {}
    assert lib.dsrt_last_error()
    # the level alone is an output, and alpha_min 1 is legal: the call gets as far as the context (which is NULL here)
    assert call(ctx=None, amin=1.0, outs=(None,) * 5 + (lev,)) == -1 and b"null argument" in lib.dsrt_last_error()
    # the convenience form: NULL arguments, sizes, patterns and bad parameters before anything else
    lo_desc = dsrt.make_desc(w, h, 4, rng_mode=1)
    ref = lambda x: C.byref(x) if x is not None else None                           # noqa: E731

    def conv(ctx=ctx, desc=lo_desc, size=(W, H), cov=(None, None), amin=0.0625, dn=None, up=P(), out=rgb, alpha=None):
        return lib.dsrt_render_upscaled_coverage_to_host(ctx, ref(desc), size[0], size[1], ref(cov[0]), ref(cov[1]), C.c_float(amin), ref(dn), ref(up), ptr(out), None, None, None,
                                                         None, ptr(alpha), None)
    grid, diag0, diag65 = dsrt.coverage_desc("grid", 4), dsrt.capi.DsrtCoverageDesc(1, 0), dsrt.capi.DsrtCoverageDesc(1, 65)
    conv_cases = {"NULL ctx": conv(ctx=None), "NULL desc": conv(desc=None), "NULL params": conv(up=None), "smaller output": conv(size=(w - 1, H)),
                  "rng_mode 0": conv(desc=dsrt.make_desc(w, h, 4, rng_mode=0)), "lo width 1": conv(desc=dsrt.make_desc(1, h, 4, rng_mode=1)),
                  "sigma NaN": conv(up=P(sigma_z=nan)), "iterations 9": conv(dn=dsrt.denoise_defaults(iterations=9)), "no output": conv(out=None),
                  "GRID at the low resolution": conv(cov=(grid, None)), "GRID at the output": conv(cov=(None, grid)), "0 samples": conv(cov=(diag0, None)),
                  "65 samples": conv(cov=(None, diag65)), "alpha_min 0": conv(amin=0.0), "alpha_min NaN": conv(amin=nan), "alpha_min 2": conv(amin=2.0),
                  "misaligned alpha": conv(alpha=a_hi.view(np.uint8)[2:])}
    assert {k: v for k, v in conv_cases.items() if v != -1} == {}
    assert all((a.view(np.uint8) == 0x5A).all() if a.dtype == np.uint8 else (a == -7.5).all() for a in everything)


@pytest.mark.parametrize("flags, says", [
    (["--rng-mode", "1", "--upscale", "2", "--coverage-aware", "--coverage", "grid:4"], "--upscale --coverage-aware takes --coverage diag:N"),
    (["--rng-mode", "0", "--upscale", "2", "--coverage-aware"], "--upscale --coverage-aware needs --rng-mode 1"),
    (["--upscale", "2", "--coverage-aware"], "--upscale --coverage-aware needs --rng-mode 1"),
    (["--rng-mode", "1", "--upscale", "2", "--coverage-aware", "0"], "ALPHA_MIN must be > 0 and <= 1"),
    (["--rng-mode", "1", "--upscale", "2", "--coverage-aware", "--temporal", "--denoise"], "does not combine"),
    (["--rng-mode", "1", "--upscale", "9", "--coverage-aware"], "between 2 and 8"),
    (["--rng-mode", "1", "--spp", "1", "--upscale", "--coverage-aware"], "--spp 2 or more"),
    (["--rng-mode", "1", "--coverage-aware"], "--coverage-aware needs --denoise or --upscale"),
])
def test_cli_usage_errors(flags, says, tmp_path):
    exe = os.path.join(ROOT, "deep-space-ray-tracer_amd", "dsrt_render")
    assert os.path.exists(exe), "build the CLI with `make tools`"
    r = subprocess.run([exe, "--obj", os.path.join(ASSETS, "station_3k.obj"), "--output_dir", str(tmp_path / "out")] + flags, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2, r.stdout + r.stderr
    assert says in r.stderr, r.stderr
    assert not (tmp_path / "out").exists()


def test_cli_usage_names_the_combination():
    exe = os.path.join(ROOT, "deep-space-ray-tracer_amd", "dsrt_render")
    r = subprocess.run([exe, "--no-such-flag"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "[--rng-mode 1 --upscale [S] --coverage-aware [ALPHA_MIN] [--coverage diag:N]]" in r.stderr


# ---- 5. quality, on the model ----
def _mse(a, ref, at):
    return float(((a.astype(np.float64) - ref)[at] ** 2).mean()) if at.any() else float("nan")


@pytest.fixture(scope="module")
def quality(dsrt, oracle):
    """Per scene, computed once: the MSE of the plain and the coverage-aware chain against 256 spp of another seed at the output size, over the sets of the tests
    below, with the native frames of the same sample budget and the level counts."""
    from test_gpu_gbuffer import expected_gbuffer
    sets = SetOracle()
    out = {}
    for name in ("station_near", "textured"):
        hs, scene, W, H, spp, depth = parity_case(dsrt, name, SEED_A)
        w, h = W // 2, H // 2
        assert (w, h, W, H) == {"station_near": (100, 56, 200, 112), "textured": (48, 32, 96, 64)}[name]
        assert spp == {"station_near": 16, "textured": 8}[name]
        S, S2 = sets.sums(scene, w, h, 0, spp)
        # the plain chain, fed as tests/test_upscale_host.py feeds it
        g_lo = {k: x for k, x in expected_gbuffer(oracle, hs, scene, w, h).items() if k in CHANNELS}
        g_hi = {k: x for k, x in expected_gbuffer(oracle, hs, scene, W, H).items() if k in CHANNELS}
        c_old, v_old = denoise(S, S2, spp, g_lo, **DENOISE_DEFAULTS)
        old, _, _ = upscale(c_old, v_old, g_lo, g_hi, **DEFAULTS)
        # the coverage-aware chain: DIAGONAL 64 at both rasters, alpha and rep
        cov_lo = CM.coverage(oracle, hs, scene, w, h, CM.DIAGONAL, 64)
        cov_hi = CM.coverage(oracle, hs, scene, W, H, CM.DIAGONAL, 64)
        cov_hi16 = CM.coverage(oracle, hs, scene, W, H, CM.DIAGONAL, 16)
        r_lo, r_hi, r_hi16 = ({k: cv["rep"][k] for k in CHANNELS} for cv in (cov_lo, cov_hi, cov_hi16))
        a_lo, a_hi = cov_lo["alpha"], cov_hi["alpha"]
        hs_b, scene_b, _, _, _, _ = parity_case(dsrt, name, SEED_B, 256)                  # (hs_b owns the arrays scene_b points into)
        ref = start(*sets.sums(scene_b, W, H, 0, 256), 256)[0]
        del scene_b, hs_b
        hs_n, scene_n, _, _, _, _ = parity_case(dsrt, name, SEED_A, spp // 4)
        Sn, S2n = sets.sums(scene_n, W, H, 0, spp // 4)
        del scene_n, hs_n
        native, _ = CM.denoise_coverage(Sn, S2n, spp // 4, {k: r_hi[k] for k in GUIDES}, a_hi, dsrt.coverage_alpha_min(), **DENOISE_DEFAULTS)     # (the native chain's own default)
        native_plain, _ = denoise(Sn, S2n, spp // 4, g_hi, **DENOISE_DEFAULTS)
        centre_hit = g_hi["range"] <= np.finfo(F).max
        where = {"partial": (a_hi > 0) & (a_hi < 1), "centre misses": ~centre_hit & (a_hi > 0), "covered": a_hi > 0, "all": np.ones((H, W), bool)}
        table = {"plain upscaler": {k: _mse(old, ref, m) for k, m in where.items()},
                 "native, coverage-denoised": {k: _mse(native, ref, m) for k, m in where.items()},
                 "native, plain denoiser": {k: _mse(native_plain, ref, m) for k, m in where.items()}}
        levels = {}
        for amin in ALPHA_MINS:
            c, v = CM.denoise_coverage(S, S2, spp, {k: r_lo[k] for k in GUIDES}, a_lo, amin, **DENOISE_DEFAULTS)
            new, _, _, level = upscale_coverage(c, v, r_lo, r_hi, a_lo, a_hi, alpha_min=amin, **DEFAULTS)
            row = f"coverage-aware, alpha_min 1/{round(1 / amin)}"
            table[row] = {k: _mse(new, ref, m) for k, m in where.items()}
            levels[row] = np.bincount(level.ravel(), minlength=4).tolist()
            if amin == ALPHA_MIN:
                assert not new[a_hi == 0].any()
                new16, _, _, level16 = upscale_coverage(c, v, r_lo, r_hi16, a_lo, cov_hi16["alpha"], alpha_min=amin, **DEFAULTS)
                table["coverage-aware, DIAGONAL 16 at the output raster"] = {k: _mse(new16, ref, m) for k, m in where.items()}
                levels["coverage-aware, DIAGONAL 16 at the output raster"] = np.bincount(level16.ravel(), minlength=4).tolist()
        counts = {k: int(m.sum()) for k, m in where.items()}
        print(f"\n{name} ({w}x{h} -> {W}x{H}, {spp} spp; native {spp // 4} spp): pixels per set {counts}")
        for row, vals in table.items():
            print(f"  {row:52s} " + "  ".join(f"{k}: {x:.6e}" for k, x in vals.items()) + (f"  levels 0..3: {levels[row]}" if row in levels else ""))
        out[name] = (table, counts, levels)
    return out


DEFAULT_ROW = f"coverage-aware, alpha_min 1/{round(1 / ALPHA_MIN)}"


def test_unmixing_beats_the_plain_upscaler_where_structure_is_thinner_than_a_pixel(quality):
    """station_near 100 x 56 -> 200 x 112 at 16 spp, against 256 spp at the output size under another seed: (a) over the output pixels with 0 < alpha_hi < 1 and
    (b) over those whose centre ray misses but alpha_hi > 0 (the plain upscaler writes these black) the coverage-aware chain's MSE is below the plain chain's.
    The measured table is in DESIGN.md section 4 and include/dsrt.h."""
    table, counts, _ = quality["station_near"]
    assert counts["partial"] >= 100 and counts["centre misses"] >= 100
    assert table[DEFAULT_ROW]["partial"] < table["plain upscaler"]["partial"]
    assert table[DEFAULT_ROW]["centre misses"] < table["plain upscaler"]["centre misses"]


@pytest.mark.parametrize("name", ["station_near", "textured"])
def test_not_worse_than_the_plain_upscaler_over_the_covered_pixels(quality, name):
    """Over all output pixels with alpha_hi > 0, and over the whole frame, with the default alpha_min, on both scenes."""
    table, _, _ = quality[name]
    assert table[DEFAULT_ROW]["covered"] <= table["plain upscaler"]["covered"]
    assert table[DEFAULT_ROW]["all"] <= table["plain upscaler"]["all"]
