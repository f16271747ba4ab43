"""The upscaler on the GPU (include/dsrt.h, UPSCALER) against the numpy model of tests/_upscale_model.py, bit for bit: synthetic two-raster frames that reach both
levels, the misses and the special values, two parity scenes rendered and denoised on the GPU, the host form, the convenience form, buffers, context state and
stream order, and the CLI.  Every float comparison is on uint32 views."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

from conftest import ASSETS, GOLDEN, ROOT
from _sample_sets import parity_case
from _denoise_model import F, tone_map
from _upscale_model import DEFAULTS, GUIDES, synthetic_pair, upscale

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

SEED = 0xDEADBEEF00001337
DEV = "cuda:0"
CHANNELS = GUIDES + ("flags",)
OUTPUTS = ("rgb8", "f32", "linear", "var", "support")


def _desc(dsrt, W, H, spp=8, depth=50, **kw):
    return dsrt.make_desc(W, H, spp, depth, seed=SEED, rng_mode=1, **kw)


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = g != w
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at {np.argwhere(bad)[0].tolist()}"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if a is not None else None


def _dev_guides(g, flags=True):
    return {k: _dev(g[k]) for k in (CHANNELS if flags else GUIDES)}


def _np_guides(g, flags=True):
    return {k: (g[k].cpu().numpy() if isinstance(g[k], torch.Tensor) else g[k]) for k in (CHANNELS if flags else GUIDES)}


def _special_pair(rng, w, h, W, H):
    """The synthetic pair with everything that takes another path: low-resolution and output misses (the scene's own), output pixels whose normal no tap shares
    (level 2), a NaN range in each raster, a low-resolution pixel of colour and variance zero."""
    c, v, lo, hi, _ = synthetic_pair(rng, w, h, W, H)
    ys, xs = np.mgrid[0:H, 0:W]
    odd = (xs % 7 == 3) & (ys % 5 == 2) & (hi["range"] < np.inf)
    hi["normal"] = np.where(odd[..., None], np.array([0, 1, 0], F), hi["normal"]).astype(F)
    hi["range"][H // 2, W // 3] = np.nan
    lo["range"][h // 2, w // 2] = np.nan
    c[0, 0] = 0
    v[0, 0] = 0
    return c, v, lo, hi


def _check_against_model(dsrt, ctx, oracle, desc, w, h, c, v, lo, hi, dc, dv, dlo, dhi, what):
    """The device form on (dc, dv, dlo, dhi) against the model on their host copies, with and without flags, with and without the variance; the tone map in
    both math modes (math_mode 1's pow is the device library's; both pows are within 2 ulp of the true one: after the 8-bit store the modes differ by one level
    at the most, as tests/test_gpu_denoise.py has it for the same tone map)."""
    params = dsrt.upscale_defaults()
    W, H = desc.width, desc.height
    desc1 = _desc(dsrt, W, H, desc.spp, desc.max_depth, math_mode=1, gamma=desc.gamma)
    for flags, with_var in itertools.product((True, False), (True, False)):
        lo_m, hi_m = ({k: g[k] for k in (CHANNELS if flags else GUIDES)} for g in (lo, hi))
        want_lin, want_var, want_sup = upscale(c, v if with_var else None, lo_m, hi_m, **DEFAULTS)
        lo_d, hi_d = ({k: g[k] for k in (CHANNELS if flags else GUIDES)} for g in (dlo, dhi))
        rgb, f32, lin, var, sup = ctx.upscale_guided(desc, w, h, dc, lo_d, hi_d, lo_var=dv if with_var else None, params=params, want_f32=True, want_var=with_var,
                                                     want_support=True)
        rgb1, _, lin1, _, sup1 = ctx.upscale_guided(desc1, w, h, dc, lo_d, hi_d, lo_var=dv if with_var else None, params=params, want_support=True)
        torch.cuda.synchronize()
        tag = (what, "flags" if flags else "no flags", "var" if with_var else "no var")
        _same(lin, want_lin, tag + ("linear",)); _same(sup, want_sup, tag + ("support",))
        if with_var:
            _same(var, want_var, tag + ("var",))
        m_rgb, m_f32 = tone_map(want_lin, desc.gamma, oracle)
        _same(rgb, m_rgb, tag + ("rgb8",)); _same(f32, m_f32, tag + ("f32",))
        _same(lin1, lin, tag + ("linear, math_mode 1",)); _same(sup1, sup, tag + ("support, math_mode 1",))
        assert int((rgb1.cpu().numpy().astype(np.int16) - rgb.cpu().numpy().astype(np.int16)).__abs__().max()) <= 1, tag
    return want_lin, want_sup


# ---- 1. synthetic frames ----
@pytest.mark.parametrize("w, h, W, H", [(37, 29, 74, 58), (37, 29, 100, 77), (2, 2, 5, 3)])
def test_synthetic_frames_equal_the_model(dsrt, gpu_ctx, oracle, w, h, W, H):
    rng = np.random.default_rng(1000 * W + H)
    c, v, lo, hi = _special_pair(rng, w, h, W, H)
    desc = _desc(dsrt, W, H)
    lin, sup = _check_against_model(dsrt, gpu_ctx, oracle, desc, w, h, c, v, lo, hi, _dev(c), _dev(v), _dev_guides(lo), _dev_guides(hi), (w, h, W, H))
    hit = hi["range"] <= np.finfo(F).max
    assert not lin[~hit].view(np.uint32).any()
    if W > 5:
        assert (hit & (sup == 0)).sum() > 10 and (sup > 0).sum() > 1000                 # both levels were exercised
    # other parameters: no normal power, wide and narrow sigmas, the sun bit off
    for changes in ({"normal_power_log2": 0, "sigma_z": 1e3, "sigma_a": 1e3}, {"normal_power_log2": 8, "sigma_z": 1e-3, "sigma_a": 1e-3}, {"use_sun": 0}):
        want = upscale(c, v, lo, hi, **{**DEFAULTS, **changes})
        _, _, g_lin, g_var, g_sup = gpu_ctx.upscale_guided(desc, w, h, _dev(c), _dev_guides(lo), _dev_guides(hi), lo_var=_dev(v), params=dsrt.upscale_defaults(**changes),
                                                           want_rgb8=False, want_var=True, want_support=True)
        torch.cuda.synchronize()
        for got, wnt, name in zip((g_lin, g_var, g_sup), want, ("linear", "var", "support")):
            _same(got, wnt, (w, h, W, H, tuple(changes), name))


# ---- 2. the parity scenes, rendered and denoised on the GPU ----
def _gbuffer(ctx, desc):
    H, W = desc.height, desc.width
    kinds = {"normal": (torch.float32, 3), "position": (torch.float32, 3), "albedo": (torch.float32, 3), "range": (torch.float32, 1), "flags": (torch.uint8, 1)}
    g = {k: torch.empty((H, W, n) if n == 3 else (H, W), dtype=dt, device=DEV) for k, (dt, n) in kinds.items()}
    torch.cuda.synchronize()
    ctx.render_gbuffer(desc, {k: x.data_ptr() for k, x in g.items()})
    torch.cuda.synchronize()
    return g


def _rendered_pair(dsrt, ctx, name, spp=8, iterations=None):
    """A parity scene at half its raster, spp samples, denoised on the GPU, and the G-buffers of both rasters: all device tensors."""
    hs, scene, W, H, _, depth = parity_case(dsrt, name, SEED, spp)
    w, h = W // 2, H // 2
    ctx.upload(scene)
    lo_desc, hi_desc = _desc(dsrt, w, h, spp, depth, gamma=scene.params.gamma), _desc(dsrt, W, H, spp, depth, gamma=scene.params.gamma)
    acc = dsrt.Accumulator(ctx, lo_desc, moments=True)
    acc.render(0)
    lo = _gbuffer(ctx, lo_desc)
    dn = dsrt.denoise_defaults() if iterations is None else dsrt.denoise_defaults(iterations=iterations)
    rgb, _, c, v = ctx.denoise_accumulated(lo_desc, acc.sum, acc.sum_sq, {k: lo[k] for k in GUIDES}, samples_done=spp, params=dn, want_var=True)
    hi = _gbuffer(ctx, hi_desc)
    return lo_desc, hi_desc, dn, rgb, c, v, lo, hi


@pytest.mark.parametrize("name, sizes", [("station_near", (100, 56, 200, 112)), ("textured", (48, 32, 96, 64))])
def test_parity_scenes_equal_the_model(dsrt, gpu_ctx, oracle, name, sizes):
    lo_desc, hi_desc, _, _, c, v, lo, hi = _rendered_pair(dsrt, gpu_ctx, name)
    assert (lo_desc.width, lo_desc.height, hi_desc.width, hi_desc.height) == sizes
    lin, sup = _check_against_model(dsrt, gpu_ctx, oracle, hi_desc, lo_desc.width, lo_desc.height, c.cpu().numpy(), v.cpu().numpy(), _np_guides(lo), _np_guides(hi),
                                    c, v, lo, hi, name)
    assert lin.any() and (sup > 0).sum() > 1000
    assert (hi["flags"].cpu().numpy() & 8).any() and not (hi["flags"].cpu().numpy() & 8).all()


# ---- 3. output subsets, inputs, refusals, context state, a side stream ----
def _raw_call(dsrt, ctx, desc, w, h, c, v, lo, hi, params, outs, stream=None, fn=None):
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None              # noqa: E731
    gl = dsrt.capi.DsrtUpscaleGuides(*[ptr(lo.get(k)) for k in CHANNELS]) if lo is not None else None
    gh = dsrt.capi.DsrtUpscaleGuides(*[ptr(hi.get(k)) for k in CHANNELS]) if hi is not None else None
    return dsrt.lib.dsrt_upscale_guided(ctx._h, C.byref(desc), w, h, ptr(c), ptr(v), C.byref(gl) if gl is not None else None, C.byref(gh) if gh is not None else None,
                                        C.byref(params) if params is not None else None, *[ptr(o) for o in outs], C.c_void_p(stream) if stream else None)


def _sentinels(W, H):
    s = lambda dt, tail: torch.full((H, W) + tail, 0x5A if dt == torch.uint8 else -7.5, dtype=dt, device=DEV)   # noqa: E731
    return [s(torch.uint8, (3,)), s(torch.float32, (3,)), s(torch.float32, (3,)), s(torch.float32, (3,)), s(torch.float32, ())]


def _untouched(outs):
    return bool((outs[0] == 0x5A).all()) and all(bool((o == -7.5).all()) for o in outs[1:])


def test_every_output_subset_inputs_refusals_and_context_state(dsrt, oracle):
    w, h, W, H = 37, 29, 100, 77
    rng = np.random.default_rng(77)
    c, v, lo, hi = _special_pair(rng, w, h, W, H)
    desc = _desc(dsrt, W, H)
    p = dsrt.upscale_defaults()
    ctx = dsrt.Context(0)
    try:
        hs, scene, W0, H0, spp0, depth0 = parity_case(dsrt, "lights", SEED)
        ctx.upload(scene)
        rdesc = _desc(dsrt, W0, H0, spp0, depth0)
        before = ctx.render_to_host(rdesc, want_f32=True)
        dc, dv, dlo, dhi = _dev(c), _dev(v), _dev_guides(lo), _dev_guides(hi)
        inputs = [dc, dv] + [dlo[k] for k in CHANNELS] + [dhi[k] for k in CHANNELS]
        keep = [t.clone() for t in inputs]
        # refusals with a scene resident, one of each class: the sentinels stay
        outs = _sentinels(W, H)
        P = dsrt.upscale_defaults
        refusals = {
            "NULL colour": _raw_call(dsrt, ctx, desc, w, h, None, dv, dlo, dhi, p, outs), "NULL lo guides": _raw_call(dsrt, ctx, desc, w, h, dc, dv, None, dhi, p, outs),
            "NULL hi channel": _raw_call(dsrt, ctx, desc, w, h, dc, dv, dlo, {**dhi, "albedo": None}, p, outs), "NULL params": _raw_call(dsrt, ctx, desc, w, h, dc, dv, dlo, dhi, None, outs),
            "rng_mode 0": _raw_call(dsrt, ctx, dsrt.make_desc(W, H, 8), w, h, dc, dv, dlo, dhi, p, outs), "shards": _raw_call(dsrt, ctx, _desc(dsrt, W, H, shard_count=2), w, h, dc, dv, dlo, dhi, p, outs),
            "lo_width 1": _raw_call(dsrt, ctx, desc, 1, h, dc, dv, dlo, dhi, p, outs), "W < lo_width": _raw_call(dsrt, ctx, desc, W + 1, h, dc, dv, dlo, dhi, p, outs),
            "H < lo_height": _raw_call(dsrt, ctx, desc, w, H + 1, dc, dv, dlo, dhi, p, outs), "normal_power_log2 9": _raw_call(dsrt, ctx, desc, w, h, dc, dv, dlo, dhi, P(normal_power_log2=9), outs),
            "sigma NaN": _raw_call(dsrt, ctx, desc, w, h, dc, dv, dlo, dhi, P(sigma_z=float("nan")), outs), "sigma 0": _raw_call(dsrt, ctx, desc, w, h, dc, dv, dlo, dhi, P(sigma_a=0.0), outs),
            "var without lo var": _raw_call(dsrt, ctx, desc, w, h, dc, None, dlo, dhi, p, outs), "no output": _raw_call(dsrt, ctx, desc, w, h, dc, dv, dlo, dhi, p, [None] * 5),
            "overlap": _raw_call(dsrt, ctx, desc, w, h, dc, dv, dlo, dhi, p, [outs[0], outs[1], outs[2], outs[2], outs[4]]),
            "output over input": _raw_call(dsrt, ctx, desc, w, h, dc, dv, dlo, dhi, p, [outs[0], None, dhi["normal"], None, None]),
        }
        assert {k: r for k, r in refusals.items() if r != -1} == {}
        torch.cuda.synchronize()
        assert _untouched(outs)
        for was, now in zip(keep, inputs):
            assert torch.equal(was.view(torch.uint8), now.view(torch.uint8))
        # all five outputs, then every subset of them: what is asked for equals the full call's, what is not keeps its sentinel
        assert _raw_call(dsrt, ctx, desc, w, h, dc, dv, dlo, dhi, p, outs) == 0
        torch.cuda.synchronize()
        want_lin, want_var, want_sup = upscale(c, v, lo, hi, **DEFAULTS)
        m_rgb, m_f32 = tone_map(want_lin, desc.gamma, oracle)
        for got, want, name in zip(outs, (m_rgb, m_f32, want_lin, want_var, want_sup), OUTPUTS):
            _same(got, want, ("all outputs", name))
        full = [o.clone() for o in outs]
        for mask in range(1, 31):
            sub = _sentinels(W, H)
            given = [s if mask >> k & 1 else None for k, s in enumerate(sub)]
            assert _raw_call(dsrt, ctx, desc, w, h, dc, dv, dlo, dhi, p, given) == 0, mask
            torch.cuda.synchronize()
            for k, name in enumerate(OUTPUTS):
                if mask >> k & 1:
                    _same(sub[k], full[k], ("subset", mask, name))
                else:
                    assert bool((sub[k] == (0x5A if k == 0 else -7.5)).all()), ("subset", mask, name, "written although not asked for")
        for was, now in zip(keep, inputs):
            assert torch.equal(was.view(torch.uint8), now.view(torch.uint8))             # the inputs are read only
        # the working memory grows and shrinks with the low-resolution frame, and a render afterwards gives the bytes it gave before
        for (w2, h2, W2, H2) in ((64, 48, 128, 96), (17, 33, 40, 70)):
            c2, v2, lo2, hi2 = _special_pair(rng, w2, h2, W2, H2)
            _, _, g_lin, g_var, g_sup = ctx.upscale_guided(_desc(dsrt, W2, H2), w2, h2, _dev(c2), _dev_guides(lo2), _dev_guides(hi2), lo_var=_dev(v2), want_rgb8=False,
                                                           want_var=True, want_support=True)
            torch.cuda.synchronize()
            for got, want, name in zip((g_lin, g_var, g_sup), upscale(c2, v2, lo2, hi2, **DEFAULTS), ("linear", "var", "support")):
                _same(got, want, (w2, h2, W2, H2, name))
        after = ctx.render_to_host(rdesc, want_f32=True)
        assert before[0].any()
        _same(after[0], before[0], "rgb8 of a render after the upscale calls"); _same(after[1], before[1], "f32 of a render after the upscale calls")
        # on a side stream, behind the work that makes its inputs on that stream
        side = torch.cuda.Stream(device=DEV)
        hc, hv = torch.from_numpy(c).pin_memory(), torch.from_numpy(v).pin_memory()
        with torch.cuda.stream(side):
            filler = torch.zeros(1 << 24, device=DEV)
            for _ in range(8):
                filler += 1.0                                                        # work in front of the copies, so that they are still queued when the call is made
            sc, sv = hc.to(DEV, non_blocking=True), hv.to(DEV, non_blocking=True)
            slo = {k: dlo[k].clone() for k in CHANNELS}
            shi = {k: dhi[k].clone() for k in CHANNELS}
            _, _, s_lin, s_var, s_sup = ctx.upscale_guided(desc, w, h, sc, slo, shi, lo_var=sv, want_rgb8=False, want_var=True, want_support=True, stream=side)
        side.synchronize()
        _same(s_lin, want_lin, "linear, side stream"); _same(s_var, want_var, "var, side stream"); _same(s_sup, want_sup, "support, side stream")
    finally:
        ctx.close()


# ---- 4. the host form and the convenience form ----
def test_host_form_equals_the_device_form(dsrt, gpu_ctx):
    w, h, W, H = 37, 29, 100, 77
    rng = np.random.default_rng(5)
    c, v, lo, hi = _special_pair(rng, w, h, W, H)
    desc = _desc(dsrt, W, H)
    for flags, with_var in ((True, True), (False, False)):
        dev = gpu_ctx.upscale_guided(desc, w, h, _dev(c), _dev_guides(lo, flags), _dev_guides(hi, flags), lo_var=_dev(v) if with_var else None, want_f32=True,
                                     want_var=with_var, want_support=True)
        torch.cuda.synchronize()
        host = gpu_ctx.upscale_guided(desc, w, h, c, _np_guides(lo, flags), _np_guides(hi, flags), lo_var=v if with_var else None, want_f32=True, want_var=with_var,
                                      want_support=True)
        for got, want, name in zip(host, dev, OUTPUTS):
            if want is None:
                assert got is None
                continue
            assert isinstance(got, np.ndarray)
            _same(got, want, ("host form", flags, name))


@pytest.mark.parametrize("iterations", [None, 3])
def test_convenience_form_is_the_five_calls(dsrt, gpu_ctx, iterations):
    """iterations None: no DsrtDenoise is given, which is the denoiser's defaults with iterations 0 -- the plain mean and variance."""
    lo_desc, hi_desc, dn, lo_rgb, c, v, lo, hi = _rendered_pair(dsrt, gpu_ctx, "station_near", iterations=iterations or 0)
    want = gpu_ctx.upscale_guided(hi_desc, lo_desc.width, lo_desc.height, c, lo, hi, lo_var=v, want_f32=True, want_var=True)
    torch.cuda.synchronize()
    rgb, f32, lin, var, got_lo, st = gpu_ctx.render_upscaled_to_host(lo_desc, hi_desc.width, hi_desc.height, denoise=dn if iterations is not None else None, want_f32=True,
                                                                     want_var=True, want_lo_rgb8=True)
    for got, w, what in zip((rgb, f32, lin, var), want, OUTPUTS):
        _same(got, w, what)
    assert rgb.shape == (hi_desc.height, hi_desc.width, 3) and rgb.any() and st.kernel_ms > 0
    _same(got_lo, lo_rgb, "the low-resolution image against the explicit chain's")
    den_rgb = gpu_ctx.render_denoised_to_host(lo_desc, params=dn)[0]
    _same(got_lo, den_rgb, "the low-resolution image against dsrt_render_denoised_to_host's")
    if iterations is None:
        _same(got_lo, gpu_ctx.render_to_host(lo_desc)[0], "without a denoiser the low-resolution image is the render")


def test_convenience_form_needs_a_scene(dsrt):
    fresh = dsrt.Context(0)
    try:
        lo_desc = _desc(dsrt, 20, 12)
        out = np.full((24, 40, 3), 0x5A, np.uint8)
        p = dsrt.upscale_defaults()
        assert dsrt.lib.dsrt_render_upscaled_to_host(fresh._h, C.byref(lo_desc), 40, 24, None, C.byref(p), C.c_void_p(out.ctypes.data), None, None, None, None, None) == -6
        assert (out == 0x5A).all()
    finally:
        fresh.close()


# ---- 5. the CLI ----
def _read_ppm(path):
    data = open(path, "rb").read()
    parts = data.split(b"\n", 3)
    w, h = map(int, parts[1].split())
    return np.frombuffer(parts[3], np.uint8).reshape(h, w, 3)


def _read_pfm(path):
    data = open(path, "rb").read()
    head, dims, scale, rest = data.split(b"\n", 3)
    w, h = map(int, dims.split())
    return np.frombuffer(rest, "<f4").reshape(h, w, 3)[::-1].reshape(h, w, 3)


def _cli(tmp, *flags, rng_mode="1"):
    exe = os.path.join(ROOT, "deep-space-ray-tracer_amd", "dsrt_render")
    cmd = [exe, "--obj", os.path.join(ASSETS, "station_3k.obj"), "--input_txt", os.path.join(GOLDEN, "rendezvous_1s_dt0_01s.txt"), "--width", "64", "--height", "48", "--spp", "8",
           "--frame", "98", "--frames", "1", "--rng-mode", rng_mode, "--output_dir", str(tmp)] + list(flags)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r


def test_cli_upscale(dsrt, gpu_ctx, tmp_path):
    W, H, spp, S = 64, 48, 8, 2
    r = _cli(tmp_path / "up", "--upscale", str(S), "--variance")
    _cli(tmp_path / "plain")
    obj = os.path.join(ASSETS, "station_3k.obj")
    hs = dsrt.HostScene().add_obj(obj)
    hs.build_bvh()
    fr = dsrt.pose_to_frame(dsrt.read_pose_file(os.path.join(GOLDEN, "rendezvous_1s_dt0_01s.txt"))[98])
    gpu_ctx.upload(hs.view(dsrt.frame_camera(fr, 40.0, W, H, spp, 50), tuple(fr.sun_dir_model)))
    desc = dsrt.make_desc(W, H, spp, 50, gamma=2.0, seed=1337, rng_mode=1)
    rgb, _, _, var, lo_rgb, _ = gpu_ctx.render_upscaled_to_host(desc, S * W, S * H, want_var=True, want_lo_rgb8=True)
    got = _read_ppm(tmp_path / "up" / "frame_0098.ppm")
    assert got.shape == (S * H, S * W, 3) and got.any()
    _same(got, rgb, "the upscaled frame")
    _same(_read_pfm(tmp_path / "up" / "frame_0098_var.pfm"), var, "the upscaled variance")
    _same(_read_ppm(tmp_path / "up" / "frame_0098_lowres.ppm"), _read_ppm(tmp_path / "plain" / "frame_0098.ppm"), "_lowres against the run without the flag")
    _same(_read_ppm(tmp_path / "up" / "frame_0098_lowres.ppm"), lo_rgb, "_lowres against the library's")
    assert f"upscale: {W} x {H} -> {S * W} x {S * H}" in r.stdout


def test_cli_upscale_with_the_denoiser_in_between(dsrt, gpu_ctx, tmp_path):
    """_lowres is the denoised frame of the run without --upscale, and the frame is the library's."""
    W, H, spp, S = 64, 48, 8, 2
    hs = dsrt.HostScene().add_obj(os.path.join(ASSETS, "station_3k.obj"))
    hs.build_bvh()
    fr = dsrt.pose_to_frame(dsrt.read_pose_file(os.path.join(GOLDEN, "rendezvous_1s_dt0_01s.txt"))[98])
    gpu_ctx.upload(hs.view(dsrt.frame_camera(fr, 40.0, W, H, spp, 50), tuple(fr.sun_dir_model)))
    desc = dsrt.make_desc(W, H, spp, 50, gamma=2.0, seed=1337, rng_mode=1)
    _cli(tmp_path / "up_dn", "--upscale", str(S), "--denoise", "2")
    _cli(tmp_path / "dn", "--denoise", "2")
    _same(_read_ppm(tmp_path / "up_dn" / "frame_0098_lowres.ppm"), _read_ppm(tmp_path / "dn" / "frame_0098.ppm"), "_lowres against the denoised run")
    want = gpu_ctx.render_upscaled_to_host(desc, S * W, S * H, denoise=dsrt.denoise_defaults(iterations=2))[0]
    _same(_read_ppm(tmp_path / "up_dn" / "frame_0098.ppm"), want, "the denoised and upscaled frame")


def test_cli_upscale_in_rng_mode_0_is_announced_and_ignored(tmp_path):
    r = _cli(tmp_path / "a", "--upscale", rng_mode="0")
    _cli(tmp_path / "b", rng_mode="0")
    assert "--upscale is not supported (post-process outside this library)" in r.stderr
    assert sorted(os.listdir(tmp_path / "a")) == sorted(os.listdir(tmp_path / "b")) == ["frame_0098.ppm"]
    assert open(tmp_path / "a" / "frame_0098.ppm", "rb").read() == open(tmp_path / "b" / "frame_0098.ppm", "rb").read()
