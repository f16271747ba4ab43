"""Temporal accumulation on the GPU (include/dsrt.h, TEMPORAL ACCUMULATION) against the numpy model of tests/_temporal_model.py, bit for bit: synthetic frames
that reach every edge, every special record and every branch of the projection, chains of three frames of two parity scenes, the three forms of the call, the
sequence the context keeps, stream order, refusals on a live context, and the CLI.  Every float comparison is on uint32 views."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ASSETS, GOLDEN, ROOT
from test_oracle import CASES, SUN
from _sample_sets import parity_case
from _denoise_model import DEFAULTS as DN, F, tone_map
import _temporal_model as model
from _temporal_model import DEFAULTS, denoise_temporal, exact_camera, random_history, wall_frame

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

SEED = 0xDEADBEEF00001337
DEV = "cuda:0"
GUIDES = ("normal", "position", "albedo", "range")
MOVES = {"station_near": [(12.8, 9.0, 37.6), (12.4, 9.0, 37.8), (12.0, 9.0, 38.0)], "textured": [(0.58, 2.0, 5.96), (0.54, 2.0, 5.98), (0.5, 2.0, 6.0)]}


def _desc(dsrt, W, H, spp=8, depth=50, seed=SEED, **kw):
    return dsrt.make_desc(W, H, spp, depth, seed=seed, rng_mode=1, **kw)


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = g != w
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at {np.argwhere(bad)[0].tolist()}"


def _camera_struct(dsrt, cam):
    """A GPUCamera of a dict of the seven vectors (tests/_temporal_model.py, exact_camera)."""
    if not isinstance(cam, dict):
        return cam
    c = dsrt.GPUCamera()
    for k, v in cam.items():
        f = getattr(c, k)
        f.x, f.y, f.z = (float(a) for a in v)
    return c


def _dev64(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).reshape(-1).view(np.int64)).to(DEV)


def _dev_guides(g):
    return {k: torch.from_numpy(np.ascontiguousarray(g[k], np.float32)).to(DEV) for k in GUIDES}


def _dev_history(h):
    return torch.from_numpy(np.ascontiguousarray(h, np.float32).reshape(-1)).to(DEV)


def _check_frame(oracle, got, want, what, gamma=2.0, rgb=True):
    """got: (rgb8, f32, linear, var, prev_xy, weight, next) as the library gives them; want: the model's dict."""
    rgb8, f32, lin, var, pxy, wgt, nxt = got
    _same(lin, want["linear"], (what, "linear")); _same(var, want["var"], (what, "var"))
    _same(np.asarray(_bits(nxt)).reshape(want["next"].shape), want["next"], (what, "next"))
    _same(pxy, want["prev_xy"], (what, "prev_xy")); _same(wgt, want["weight"], (what, "weight"))
    if rgb:
        m_rgb, m_f32 = tone_map(want["linear"], gamma, oracle)
        _same(rgb8, m_rgb, (what, "rgb8")); _same(f32, m_f32, (what, "f32"))


# ---- 1. synthetic frames: no scene ----
SIZES = [(2, 2), (3, 7), (5, 5), (17, 33), (37, 29), (64, 2)]


def _synthetic(dsrt, rng, W, H):
    """{kind: (S, S2, n, guides, previous camera, previous history, parameter changes)}: one frame for each thing that can go wrong."""
    look = lambda p: dsrt.camera_look_at(p, (0, 0, 0), 40.0, W, H, 8, 5)              # noqa: E731
    cam1 = look((0.0, 0.0, 10.2))
    shift = lambda: look((float(rng.uniform(-0.6, 0.6)), float(rng.uniform(-0.6, 0.6)), float(rng.uniform(9.0, 11.0))))   # noqa: E731
    out = {}
    cam0 = shift()
    S, S2, n, g = wall_frame(rng, cam1, W, H, miss=0.2)
    prev, _ = random_history(rng, wall_frame(rng, cam0, W, H)[3], special=0.3)
    out["moved camera, rejected records sprinkled in"] = (S, S2, n, g, cam0, prev, {})
    out["the first frame"] = (S, S2, n, g, None, None, {})
    n2 = n.copy(); n2[0] = 1; n2[H - 1] = 0; n2[H // 2, ::2] = 3
    out["rows of n < 2, per-pixel counts"] = (S, S2, n2, g, cam0, prev, {})
    cam0 = shift()
    S, S2, n, g = wall_frame(rng, cam1, W, H)
    prev, _ = random_history(rng, wall_frame(rng, cam0, W, H)[3])
    X = g["position"].copy()
    kind = rng.integers(0, 12, size=(H, W))
    o = np.array([cam0.origin.x, cam0.origin.y, cam0.origin.z], F)
    X[kind == 1] = np.nan
    X[kind == 2] = np.inf
    X[kind == 3] = o                                                                # cc = 0
    X[kind == 4] = o + np.array([0, 0, 5], F)                                       # behind the previous camera
    X[kind == 5] *= F(40)                                                           # on the plane, far outside the previous image
    n3 = n.copy()
    n3[(kind == 1) | (kind == 2)] = 1                                               # (guides must be finite where a pixel is filtered; with n < 2 it is still projected)
    out["positions that do not project"] = (S, S2, n3, {**g, "position": X}, cam0, prev, {})
    # a camera of exact numbers and points on the bounds of the image test (exactly on them where W - 1 is a power of two)
    S, S2, n, g = wall_frame(rng, cam1, W, H)
    xs = np.array([-0.5, W - 1.0, float(W), -1.0, 0.0, W - 0.5, (W - 1) / 2, -0.999, W - 1e-3], F)
    ys = np.array([-0.5, H - 1.0, float(H), -1.0, 0.0, H - 0.5, (H - 1) / 2, -0.999, H - 1e-3], F)
    fx, fy = xs[rng.integers(0, len(xs), size=(H, W))], ys[rng.integers(0, len(ys), size=(H, W))]
    X = np.stack([(fx + F(0.5)) / F(W - 1) * F(2) - F(1), (F(H - 1) - fy + F(0.5)) / F(H - 1) * F(2) - F(1), np.full((H, W), -1, F)], -1).astype(F)
    ge = {"normal": np.broadcast_to(np.array([0, 0, 1], F), (H, W, 3)).copy(), "position": X, "albedo": g["albedo"], "range": np.full((H, W), 1.5, F)}
    prev, _ = random_history(rng, ge, special=0.1)
    out["points on the bounds of the image test"] = (S, S2, n, ge, exact_camera(), prev, {"min_support": 0.25})
    cam0 = shift()
    S, S2, n, g = wall_frame(rng, cam1, W, H, miss=0.1)
    prev, _ = random_history(rng, wall_frame(rng, cam0, W, H)[3], special=0.15)
    out["alpha_min 0"] = (S, S2, n, g, cam0, prev, {"alpha_min": 0.0})
    out["alpha_min 1"] = (S, S2, n, g, cam0, prev, {"alpha_min": 1.0})
    out["one tap is enough, any normal"] = (S, S2, n, g, cam0, prev, {"min_support": 1e-3, "normal_cos_min": -1.0})
    out["everything must agree"] = (S, S2, n, g, cam0, prev, {"min_support": 1.0, "normal_cos_min": 1.0, "plane_tol": 1e-6})
    # a camera that has not moved: every tap of weight >= 0.99 on the pixel's own surface waives the occluder guard that the off-plane records raise
    S, S2, n, g = wall_frame(rng, cam1, W, H, miss=0.1)
    prev, _ = random_history(rng, wall_frame(rng, cam1, W, H)[3], special=0.1)
    out["a camera that has not moved"] = (S, S2, n, g, cam1, prev, {})
    return out


@pytest.mark.parametrize("W, H", SIZES)
def test_synthetic_frames_equal_the_model(dsrt, gpu_ctx, oracle, W, H):
    rng = np.random.default_rng(1000 * W + H)
    desc = _desc(dsrt, W, H)
    blended = voided = waived = 0
    for kind, (S, S2, n, g, cam, prev, changes) in _synthetic(dsrt, rng, W, H).items():
        tp = {**DEFAULTS, **changes}
        for it in (0, 3):
            want = denoise_temporal(S, S2, n, g, cam, prev, temporal=tp, **{**DN, "iterations": it})
            got = gpu_ctx.denoise_temporal_to_host(desc, S, S2, g, _camera_struct(dsrt, cam) if cam is not None else None, prev, n=n, temporal=dsrt.temporal_defaults(**changes),
                                                   params=dsrt.denoise_defaults(iterations=it), want_f32=True, want_var=True)
            _check_frame(oracle, got, want, (W, H, kind, it))
        blended += int(want["found"].sum())
        if cam is not None:                                                          # the occluder guard: pixels it voids, and pixels where a tap waives it
            info = model.INFO
            voided += int((info["supported"] & info["guarded"] & ~info["seen"]).sum())
            waived += int((info["supported"] & info["guarded"] & info["seen"]).sum())
        if kind == "the first frame":
            assert not want["found"].any() and (_bits(want["prev_xy"]) == 0x7FC00000).all()
        if kind == "alpha_min 1" and W * H > 100:
            assert want["found"].sum() > 20
    assert blended > (W * H) // 2, "the synthetic frames of this size blend next to nothing"
    assert W * H <= 100 or (voided > 0 and waived > 0), "the synthetic frames of this size do not reach the occluder guard and its waiver"


# ---- 2. chains of three frames of two parity scenes ----
@pytest.mark.parametrize("name", ["station_near", "textured"])
def test_scene_chain_equals_the_model(dsrt, gpu_ctx, oracle, name):
    world, (_, lookat, vfov, W, H, depth), spp = CASES[name]
    hs, scene, _, _, _, _ = parity_case(dsrt, name, SEED)
    gpu_ctx.upload(scene)
    gamma = 2.0                                                                     # make_desc's
    td = dsrt.TemporalDenoiser(gpu_ctx, _desc(dsrt, W, H, spp, depth))
    prev = prev_cam = None
    found = 0
    for f, lookfrom in enumerate(MOVES[name]):
        cam = dsrt.camera_look_at(lookfrom, lookat, vfov, W, H, spp, depth)
        gpu_ctx.set_camera_sun(cam, SUN)
        desc = _desc(dsrt, W, H, spp, depth, seed=SEED + f)
        acc = dsrt.Accumulator(gpu_ctx, desc, moments=True)
        acc.render(0)
        g = acc.guides()
        before, hist_prev = td.current, (td.history[td.current].clone() if f else None)
        rgb, f32, lin, var, pxy, wgt = td.step(acc, cam, guides=g, want_f32=True, want_var=True, want_prev_xy=True, want_weight=True)
        # math_mode 1 on the same sums, guides and history: the same linear, var and next; the bytes within one level
        desc1 = _desc(dsrt, W, H, spp, depth, seed=SEED + f, math_mode=1)
        next1 = torch.empty_like(td.history[0])
        rgb1, _, lin1, var1, _, _ = gpu_ctx.denoise_temporal(desc1, acc.sum, acc.sum_sq, g, next1, prev_cam, hist_prev, samples_done=spp, want_var=True)
        torch.cuda.synchronize()
        assert td.current == (before ^ 1 if f else before)
        S, S2 = acc.sum.cpu().numpy().view(np.uint64).reshape(H, W, 3), acc.sum_sq.cpu().numpy().view(np.uint64).reshape(H, W, 3)
        gh = {k: x.cpu().numpy() for k, x in g.items()}
        want = denoise_temporal(S, S2, spp, gh, prev_cam, prev, **DN)
        _check_frame(oracle, (rgb, f32, lin, var, pxy, wgt, td.history[td.current]), want, (name, f), gamma)
        _same(lin1, lin, (name, f, "linear, math_mode 1")); _same(var1, var, (name, f, "var, math_mode 1")); _same(next1, td.history[td.current], (name, f, "next, math_mode 1"))
        assert int((rgb1.cpu().numpy().astype(np.int16) - rgb.cpu().numpy().astype(np.int16)).__abs__().max()) <= 1, (name, f)
        prev, prev_cam = want["next"], cam
        found += int(want["found"].sum()) if f else 0
    assert found > 2000, "the chain found next to no history"


# ---- 3. the forms of the call ----
def _textured_frame(dsrt, ctx, f, spp=8):
    """Frame f of the textured chain rendered on ctx: (desc, cam, acc, guides)."""
    _, (_, lookat, vfov, W, H, depth), _ = CASES["textured"]
    cam = dsrt.camera_look_at(MOVES["textured"][f], lookat, vfov, W, H, spp, depth)
    ctx.set_camera_sun(cam, SUN)
    desc = _desc(dsrt, W, H, spp, depth, seed=SEED + f)
    acc = dsrt.Accumulator(ctx, desc, moments=True)
    acc.render(0)
    return desc, cam, acc, acc.guides()


def test_first_frame_is_the_plain_denoiser_and_the_host_form_is_the_device_form(dsrt, gpu_ctx):
    hs, scene, W, H, _, _ = parity_case(dsrt, "textured", SEED)
    gpu_ctx.upload(scene)
    desc, cam0, acc, g = _textured_frame(dsrt, gpu_ctx, 0)
    p = dsrt.denoise_defaults(iterations=3)
    hist = [torch.zeros(W * H * 16, dtype=torch.float32, device=DEV) for _ in range(2)]
    first = gpu_ctx.denoise_temporal(desc, acc.sum, acc.sum_sq, g, hist[0], samples_done=desc.spp, params=p, want_f32=True, want_var=True, want_prev_xy=True, want_weight=True)
    plain = gpu_ctx.denoise_accumulated(desc, acc.sum, acc.sum_sq, g, samples_done=desc.spp, params=p, want_f32=True, want_var=True)
    torch.cuda.synchronize()
    for got, want, what in zip(first[:4], plain, ("rgb8", "f32", "linear", "var")):
        _same(got, want, ("prev = NULL against dsrt_denoise_accumulated", what))
    assert (_bits(first[4]) == 0x7FC00000).all()
    filt = torch.isfinite(g["range"])
    assert bool((first[5][filt] == desc.spp).all()) and not bool(first[5][~filt].any())
    # the second frame, device form against host form
    desc, cam1, acc, g = _textured_frame(dsrt, gpu_ctx, 1)
    dev = gpu_ctx.denoise_temporal(desc, acc.sum, acc.sum_sq, g, hist[1], cam0, hist[0], samples_done=desc.spp, params=p, want_f32=True, want_var=True, want_prev_xy=True, want_weight=True)
    torch.cuda.synchronize()
    host = gpu_ctx.denoise_temporal_to_host(desc, acc.sum.cpu().numpy().view(np.uint64), acc.sum_sq.cpu().numpy().view(np.uint64), {k: x.cpu().numpy() for k, x in g.items()}, cam0,
                                            hist[0].cpu().numpy(), samples_done=desc.spp, params=p, want_f32=True, want_var=True)
    for got, want, what in zip(host, dev + (hist[1].reshape(H, W, 16),), ("rgb8", "f32", "linear", "var", "prev_xy", "weight", "next")):
        _same(got, want, ("host form against device form", what))
    assert not bool(torch.isnan(dev[4]).all()) and bool((dev[5] > desc.spp).any())


def test_convenience_form_is_the_explicit_chain(dsrt, gpu_ctx):
    """dsrt_render_denoised_temporal_to_host keeps the sequence in the context: equal to the explicit chain frame by frame; reset, another size and a new upload each
    start a new sequence; a clone has its own."""
    hs, scene, W, H, _, _ = parity_case(dsrt, "textured", SEED)
    ctx = dsrt.Context(0)
    clone = None
    try:
        ctx.upload(scene)
        td = dsrt.TemporalDenoiser(ctx, _desc(dsrt, W, H))
        p = dsrt.denoise_defaults(iterations=2)

        def explicit(f):
            desc, cam, acc, g = _textured_frame(dsrt, ctx, f)
            out = td.step(acc, cam, guides=g, params=p, want_f32=True, want_var=True, want_prev_xy=True)
            torch.cuda.synchronize()
            return desc, out

        def conv(desc, what, want, **kw):
            got = ctx.render_denoised_temporal_to_host(desc, params=p, want_f32=True, want_var=True, want_prev_xy=True, **kw)
            for a, b, ch in zip(got[:5], want[:5], ("rgb8", "f32", "linear", "var", "prev_xy")):
                _same(a, b, (what, ch))
            assert got[5].kernel_ms > 0
            return got

        for f in range(3):
            desc, want = explicit(f)                                                # (sets the frame's camera on ctx)
            got = conv(desc, ("frame", f), want, reset=(f == 0))
            assert bool(np.isnan(got[4]).all()) == (f == 0)
        # reset: frame 2 again, without history -- the explicit chain restarted
        td.reset()
        desc, want = explicit(2)
        assert bool(torch.isnan(want[4]).all())
        conv(desc, "reset", want, reset=True)
        # a clone has its own sequence (none yet) and leaves this context's alone
        clone = ctx.clone()
        clone.set_camera_sun(dsrt.camera_look_at(MOVES["textured"][1], CASES["textured"][1][1], CASES["textured"][1][2], W, H, 8, 50), SUN)
        d1 = _desc(dsrt, W, H, 8, desc.max_depth, seed=SEED + 1)
        c_first = clone.render_denoised_temporal_to_host(d1, params=p, want_prev_xy=True)
        assert np.isnan(c_first[4]).all() and c_first[0].any()
        desc, want = explicit(1)                                                    # ctx goes on from its frame 2: history
        got = conv(desc, "after the clone's call", want)
        assert not np.isnan(got[4]).all()
        # another size starts a new sequence, and so does the size changing back
        small = _desc(dsrt, 48, 32, 8, desc.max_depth, seed=SEED)
        assert np.isnan(ctx.render_denoised_temporal_to_host(small, params=p, want_prev_xy=True)[4]).all()
        td.reset()
        desc, want = explicit(0)
        conv(desc, "after another size", want)
        desc, want = explicit(1)
        assert not np.isnan(conv(desc, "the sequence goes on", want)[4]).all()
        # a new upload starts a new sequence
        ctx.upload(scene)
        td.reset()
        desc, want = explicit(2)
        assert np.isnan(conv(desc, "after an upload", want)[4]).all()
        # before an upload: DSRT_ERR_NO_SCENE, nothing written
        fresh = dsrt.Context(0)
        try:
            out = np.zeros((H, W, 3), np.uint8)
            rc = dsrt.lib.dsrt_render_denoised_temporal_to_host(fresh._h, C.byref(desc), C.byref(p), C.byref(dsrt.temporal_defaults()), 0, C.c_void_p(out.ctypes.data), None, None,
                                                                None, None, None)
            assert rc == -6 and not out.any()
        finally:
            fresh.close()
    finally:
        if clone is not None:
            clone.close()
        ctx.close()


# ---- 4. stream order and refusals on a live context ----
def _raw_call(dsrt, ctx, desc, S, S2, g, cam, prev, nxt, tp, dn, outs, pxy, wgt, done=8, stream=None):
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None              # noqa: E731
    acc = dsrt.capi.DsrtAccum(ptr(S), ptr(S2))
    gd = dsrt.capi.DsrtDenoiseGuides(*[ptr(g[k]) for k in GUIDES])
    return dsrt.lib.dsrt_denoise_temporal(ctx._h, C.byref(desc), C.byref(acc), done, None, C.byref(gd), C.byref(cam) if cam is not None else None, ptr(prev), ptr(nxt),
                                          C.byref(tp) if tp is not None else None, C.byref(dn), *[ptr(o) for o in outs], ptr(pxy), ptr(wgt), C.c_void_p(stream) if stream else None)


def test_refusals_leave_buffers_alone_and_a_side_stream_keeps_order(dsrt, gpu_ctx):
    W, H = 37, 29
    rng = np.random.default_rng(78)
    cam0 = dsrt.camera_look_at((0.3, -0.2, 10.0), (0, 0, 0), 40.0, W, H, 8, 5)
    cam1 = dsrt.camera_look_at((0.0, 0.0, 10.2), (0, 0, 0), 40.0, W, H, 8, 5)
    S, S2, n, g = wall_frame(rng, cam1, W, H, miss=0.1)
    prev, _ = random_history(rng, wall_frame(rng, cam0, W, H)[3], special=0.1)
    desc = _desc(dsrt, W, H)
    dn, tp = dsrt.denoise_defaults(iterations=3), dsrt.temporal_defaults()
    want = denoise_temporal(S, S2, 8, g, cam0, prev, **{**DN, "iterations": 3})
    assert want["found"].sum() > 300
    dS, dS2, dg, dprev = _dev64(S), _dev64(S2), _dev_guides(g), _dev_history(prev)
    keep = [dS.clone(), dS2.clone(), dprev.clone()] + [dg[k].clone() for k in GUIDES]
    sentinel = lambda dt, shape=(H, W, 3): torch.full(shape, 0x5A if dt == torch.uint8 else -7.5, dtype=dt, device=DEV)   # noqa: E731
    outs = [sentinel(torch.uint8), sentinel(torch.float32), sentinel(torch.float32), sentinel(torch.float32)]
    nxt, pxy, wgt = sentinel(torch.float32, (H * W * 16,)), sentinel(torch.float32, (H, W, 2)), sentinel(torch.float32, (H, W))
    T = dsrt.temporal_defaults
    call = lambda **kw: _raw_call(dsrt, gpu_ctx, **{**dict(desc=desc, S=dS, S2=dS2, g=dg, cam=cam0, prev=dprev, nxt=nxt, tp=tp, dn=dn, outs=outs, pxy=pxy, wgt=wgt), **kw})   # noqa: E731
    refusals = {
        "NULL sum_sq": call(S2=None), "rng_mode 0": call(desc=dsrt.make_desc(W, H, 8)), "iterations 7": call(dn=dsrt.denoise_defaults(iterations=7)),
        "camera without history": call(prev=None), "history without camera": call(cam=None), "NULL next": call(nxt=None), "NULL DsrtTemporal": call(tp=None),
        "alpha_min 2": call(tp=T(alpha_min=2.0)), "normal_cos_min -2": call(tp=T(normal_cos_min=-2.0)), "plane_tol 0": call(tp=T(plane_tol=0.0)),
        "min_support NaN": call(tp=T(min_support=float("nan"))), "min_support 1.5": call(tp=T(min_support=1.5)),
        "next misaligned": call(nxt=nxt[1:]), "prev misaligned": call(prev=dprev[2:]), "next is prev": call(nxt=dprev), "next over an input": call(nxt=dg["position"]),
        "next over an output": call(outs=[outs[0], outs[1], nxt, outs[3]]), "prev_xy over next": call(pxy=nxt), "weight over prev": call(wgt=dprev),
    }
    assert {k: v for k, v in refusals.items() if v != -1} == {}
    torch.cuda.synchronize()
    assert (outs[0] == 0x5A).all() and all((o == -7.5).all() for o in outs[1:] + [nxt, pxy, wgt])
    for was, now in zip(keep, [dS, dS2, dprev] + [dg[k] for k in GUIDES]):
        assert torch.equal(was.view(torch.uint8), now.view(torch.uint8))
    # the call itself: every output element written, every input untouched
    assert call() == 0
    torch.cuda.synchronize()
    _same(outs[2], want["linear"], "linear"); _same(outs[3], want["var"], "var"); _same(nxt.reshape(H, W, 16), want["next"], "next")
    _same(pxy, want["prev_xy"], "prev_xy"); _same(wgt, want["weight"], "weight")
    assert not (outs[1] == -7.5).any() and not (outs[0] == 0x5A).all()
    for was, now in zip(keep, [dS, dS2, dprev] + [dg[k] for k in GUIDES]):
        assert torch.equal(was.view(torch.uint8), now.view(torch.uint8))
    # asynchronous, on a side stream: the call is made while the work that makes its inputs is still queued there, between two renders of the same context
    hs, scene, RW, RH, rspp, rdepth = parity_case(dsrt, "textured", SEED)
    gpu_ctx.upload(scene)
    rdesc = _desc(dsrt, RW, RH, rspp, rdepth)
    ref = gpu_ctx.render_to_host(rdesc)[0]
    side = torch.cuda.Stream(device=DEV)
    hS, hS2 = (torch.from_numpy(a.reshape(-1).view(np.int64)).pin_memory() for a in (S, S2))
    hprev = torch.from_numpy(prev.reshape(-1)).pin_memory()
    before, after = torch.zeros((RH, RW, 3), dtype=torch.uint8, device=DEV), torch.zeros((RH, RW, 3), dtype=torch.uint8, device=DEV)
    nxt2 = torch.zeros(H * W * 16, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        filler = torch.zeros(1 << 24, device=DEV)
        for _ in range(8):
            filler += 1.0                                                            # work in front of the copies, so that they are still queued when the call is made
        sS, sS2, sprev = hS.to(DEV, non_blocking=True), hS2.to(DEV, non_blocking=True), hprev.to(DEV, non_blocking=True)
        sg = {k: (dg[k] * 1.0) for k in GUIDES}
        gpu_ctx.render(rdesc, before.data_ptr(), stream=side.cuda_stream)
        _, _, lin, var, spxy, swgt = gpu_ctx.denoise_temporal(desc, sS, sS2, sg, nxt2, cam0, sprev, samples_done=8, params=dn, want_rgb8=False, want_var=True, want_prev_xy=True,
                                                              want_weight=True, stream=side)
        gpu_ctx.render(rdesc, after.data_ptr(), stream=side.cuda_stream)
    side.synchronize()
    _same(lin, want["linear"], "linear, side stream"); _same(var, want["var"], "var, side stream"); _same(nxt2.reshape(H, W, 16), want["next"], "next, side stream")
    _same(spxy, want["prev_xy"], "prev_xy, side stream"); _same(swgt, want["weight"], "weight, side stream")
    assert ref.any()
    _same(before, ref, "the render queued before the call"); _same(after, ref, "the render queued after the call")


# ---- 5. the CLI ----
def _read_ppm(path):
    data = open(path, "rb").read()
    parts = data.split(b"\n", 3)
    w, h = map(int, parts[1].split())
    return np.frombuffer(parts[3], np.uint8).reshape(h, w, 3)


def _read_pfm(path):
    data = open(path, "rb").read()
    head, dims, scale, rest = data.split(b"\n", 3)
    assert head == b"PF"
    w, h = map(int, dims.split())
    return np.frombuffer(rest, "<f4").reshape(h, w, 3)[::-1].reshape(h, w, 3)


def test_cli_temporal_and_flow(dsrt, gpu_ctx, tmp_path):
    exe = os.path.join(ROOT, "deep-space-ray-tracer_amd", "dsrt_render")
    obj = os.path.join(ASSETS, "station_3k.obj")
    poses_txt = os.path.join(GOLDEN, "rendezvous_1s_dt0_01s.txt")
    W, H, spp, it, first = 96, 64, 8, 2, 96
    base = [exe, "--obj", obj, "--input_txt", poses_txt, "--width", str(W), "--height", str(H), "--spp", str(spp), "--frame", str(first), "--frames", "3", "--rng-mode", "1",
            "--denoise", str(it)]
    out_t, out_p = tmp_path / "temporal", tmp_path / "plain"
    r = subprocess.run(base + ["--output_dir", str(out_t), "--temporal", "--flow"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r2 = subprocess.run(base + ["--output_dir", str(out_p)], capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0, r2.stdout + r2.stderr
    hs = dsrt.HostScene().add_obj(obj)
    hs.build_bvh()
    poses = dsrt.read_pose_file(poses_txt)
    p = dsrt.denoise_defaults(iterations=it)
    ys, xs = np.mgrid[0:H, 0:W]
    moved = 0
    for k, i in enumerate(range(first, first + 3)):
        fr = dsrt.pose_to_frame(poses[i])
        cam = dsrt.frame_camera(fr, 40.0, W, H, spp, 50)
        if k == 0:
            gpu_ctx.upload(hs.view(cam, tuple(fr.sun_dir_model)))
        gpu_ctx.set_camera_sun(cam, tuple(fr.sun_dir_model))
        desc = dsrt.make_desc(W, H, spp, 50, gamma=2.0, seed=1337 + i, rng_mode=1)
        rgb, _, _, _, pxy, _ = gpu_ctx.render_denoised_temporal_to_host(desc, params=p, reset=(k == 0), want_prev_xy=True)
        raw = gpu_ctx.render_to_host(desc)[0]
        stem = f"frame_{i:04d}"
        _same(_read_ppm(out_t / f"{stem}.ppm"), rgb, (i, "the temporal frame"))
        _same(_read_ppm(out_t / f"{stem}_raw.ppm"), raw, (i, "the raw frame"))
        flow = np.stack([pxy[..., 0] - xs.astype(F), pxy[..., 1] - ys.astype(F), np.zeros((H, W), F)], -1).astype(F)
        got = _read_pfm(out_t / f"{stem}_flow.pfm")
        assert np.array_equal(np.isnan(got), np.isnan(flow)) and np.array_equal(got[~np.isnan(got)].view(np.uint32), flow[~np.isnan(flow)].view(np.uint32)), (i, "flow")
        assert np.isnan(flow[..., 0]).all() == (k == 0) and rgb.any() and (rgb != raw).any()
        moved += int(np.nansum(np.abs(flow)) > 0) if k else 0
        # without --temporal: seed 1337 for every frame, dsrt_render_denoised_to_host's image -- what --denoise gave before the flag existed
        d0 = dsrt.make_desc(W, H, spp, 50, gamma=2.0, seed=1337, rng_mode=1)
        plain = gpu_ctx.render_denoised_to_host(d0, params=p)[0]
        _same(_read_ppm(out_p / f"{stem}.ppm"), plain, (i, "--denoise alone"))
        _same(_read_ppm(out_p / f"{stem}_raw.ppm"), gpu_ctx.render_to_host(d0)[0], (i, "--denoise alone, raw"))
        assert not (out_p / f"{stem}_flow.pfm").exists()
    assert moved == 2
    assert f"denoise: {it} iterations, temporal, seed {1337 + first}" in r.stdout and "iterations, temporal" not in r2.stdout
