"""The coverage pass and the coverage-aware denoiser on the GPU (include/dsrt.h, COVERAGE and COVERAGE DEMODULATION) against tests/_coverage_model.py, bit for bit:
every output against buffers built per sub-sample from the oracle's camera ray and scene_hit, the representative against the G-buffer pass, classes on scenes
with bodies, the calls' envelope and refusals, the demodulated filter against the numpy model, the convenience form and the CLI.  Every float comparison is on
uint32 views."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _bodies_shapes as S
import _coverage_model as M
from conftest import ASSETS, GOLDEN, ROOT, load_world
from test_oracle import CASES, SUN
from _sample_sets import parity_case
from _denoise_model import DEFAULTS, F, denoise, synthetic_frame, tone_map

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

SEED = 0xDEADBEEF00001337
DEV = "cuda:0"
GUIDES = ("normal", "position", "albedo", "range")
OWN = ("hits", "alpha", "mask", "sun_hits", "sun_alpha", "sun_mask")
GRID, DIAG = M.GRID, M.DIAGONAL
# the rasters that carry the index arithmetic: on 13 x 7 and 11 x 5 pixel groups wrap rows and the last workgroup is partly empty (n = 9, 25, 49: P = 7, 2, 1;
# n = 33: P = 1 with 31 idle lanes); DIAGONAL 64 (a wave per pixel) only here, to keep the oracle's loop within seconds
SMALL = {(13, 7): [(GRID, 1), (GRID, 2), (GRID, 3), (GRID, 5), (GRID, 8), (DIAG, 1), (DIAG, 7), (DIAG, 33), (DIAG, 64)],
         (11, 5): [(GRID, 3), (GRID, 5), (GRID, 7), (DIAG, 33), (DIAG, 64)]}
LARGER = (50, 28)


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = g != w
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at {np.argwhere(bad)[0].tolist()}"


def _same_coverage(got, want, what, keys=OWN, rep=M.GB_KEYS):
    for k in keys:
        _same(got[k], want[k], (what, k))
    for k in rep:
        _same(got["rep"][k], want["rep"][k], (what, "rep", k))


def _cd(dsrt, pattern, samples):
    return dsrt.coverage_desc(pattern, samples)


def _scene(dsrt, name, W, H):
    world, (lookfrom, lookat, vfov, _, _, depth), spp = CASES[name]
    hs = load_world(dsrt, world)
    return hs, hs.view(dsrt.camera_look_at(lookfrom, lookat, vfov, W, H, spp, depth), SUN)


# ---- 1. against the oracle ----
@pytest.mark.parametrize("size", sorted(SMALL))
@pytest.mark.parametrize("name", sorted(CASES))
def test_every_output_matches_the_oracle_on_the_small_rasters(dsrt, gpu_ctx, oracle, name, size):
    W, H = size
    hs, scene = _scene(dsrt, name, W, H)
    gpu_ctx.upload(scene)
    desc = dsrt.make_desc(W, H, 1)
    any_hit = False
    for pattern, samples in SMALL[size]:
        got = gpu_ctx.coverage_to_host(desc, _cd(dsrt, pattern, samples), rep=True)
        want = M.coverage(oracle, hs, scene, W, H, pattern, samples)
        _same_coverage(got, want, (name, size, pattern, samples))
        any_hit |= bool(want["hits"].any())
    assert any_hit


@pytest.mark.parametrize("name", ["station_near", "mixed"])
def test_every_output_matches_the_oracle_on_a_larger_raster(dsrt, gpu_ctx, oracle, name):
    W, H = LARGER
    hs, scene = _scene(dsrt, name, W, H)
    gpu_ctx.upload(scene)
    desc = dsrt.make_desc(W, H, 1)
    for pattern, samples in ((GRID, 2), (GRID, 3), (DIAG, 7)):
        got = gpu_ctx.coverage_to_host(desc, _cd(dsrt, pattern, samples), rep=True)
        want = M.coverage(oracle, hs, scene, W, H, pattern, samples)
        _same_coverage(got, want, (name, pattern, samples))
        n = M.count(pattern, samples)
        assert ((want["hits"] > 0) & (want["hits"] < n)).sum() > 20 and (want["sun_hits"] > 0).any() and (want["sun_hits"] < want["hits"]).any()


# ---- 2. against the G-buffer pass ----
def test_one_sample_is_the_gbuffer_and_an_odd_count_is_where_the_centre_hits(dsrt, gpu_ctx):
    W, H = 97, 55
    hs, scene = _scene(dsrt, "station_near", W, H)
    gpu_ctx.upload(scene)
    desc = dsrt.make_desc(W, H, 1)
    gb = gpu_ctx.gbuffer_to_host(desc)
    centre = (gb["flags"] & 1).astype(bool)
    assert centre.any() and not centre.all()
    for pattern in (GRID, DIAG):
        got = gpu_ctx.coverage_to_host(desc, _cd(dsrt, pattern, 1), rep=True)
        for k in M.GB_KEYS:
            _same(got["rep"][k], gb[k], ("samples = 1", pattern, k))
        _same(got["hits"], centre.astype(np.uint8), "hits of one sample")
        _same(got["mask"], centre.astype(np.uint64), "mask of one sample")
        _same(got["sun_hits"], ((gb["flags"] & 8) != 0).astype(np.uint8), "sun_hits of one sample")
    for pattern, samples in ((GRID, 3), (GRID, 5), (GRID, 7), (DIAG, 7), (DIAG, 33), (DIAG, 63)):
        got = gpu_ctx.coverage_to_host(desc, _cd(dsrt, pattern, samples), rep=True)
        for k in M.GB_KEYS:
            _same(got["rep"][k][centre], gb[k][centre], ("odd count", pattern, samples, k))
        outside = ~centre & (got["hits"] > 0)                            # the pixels the G-buffer calls empty and the samples do not
        assert outside.any() and (got["rep"]["flags"][outside] & 1).all() and np.isfinite(got["rep"]["range"][outside]).all()
        assert not got["rep"]["flags"][got["hits"] == 0].any()


# ---- 3. classes ----
def _classes_case(dsrt, ctx, oracle, name, posed, W, H, pattern, samples):
    rest = S.build(dsrt, name)
    host = S.build(dsrt, name)
    if posed:
        S.apply(host, S.poses(name))
    cam = S.camera(dsrt, host, W, H)
    ctx.upload_bodies(rest, rest.view(cam, S.SUN))
    if posed:
        S.apply(ctx, S.poses(name))
    ranges = S.ranges(host)
    desc = dsrt.make_desc(W, H, 1)
    got = ctx.coverage_to_host(desc, _cd(dsrt, pattern, samples), rep=("prim_id", "flags"), classes=dsrt.coverage_classes(ranges))
    want = M.coverage(oracle, host, host.view(cam, S.SUN), W, H, pattern, samples, classes=ranges)
    _same_coverage(got, want, (name, "classes"), keys=OWN + ("class_hits",), rep=("prim_id", "flags"))
    ch = got["class_hits"].astype(np.int64)
    assert ch.shape == (H, W, len(ranges)) and (ch.sum(axis=2) <= got["hits"]).all()
    _same(ch.sum(axis=2).astype(np.uint8), got["hits"], "the bodies partition the triangles: their counts add up to hits")
    return ranges, ch


def test_classes_on_a_scene_with_empty_bodies(dsrt, gpu_ctx, oracle):
    ranges, ch = _classes_case(dsrt, gpu_ctx, oracle, "holes", False, 31, 17, GRID, 3)
    empty = [b for b, (_, num) in enumerate(ranges) if num == 0]
    assert empty == [1, 3, 5] and not ch[..., empty].any() and all(ch[..., b].any() for b in (0, 2, 4))


def test_classes_follow_a_pose_update(dsrt, gpu_ctx, oracle):
    ranges, ch = _classes_case(dsrt, gpu_ctx, oracle, "leaves_only", True, 31, 17, DIAG, 9)
    assert sum(bool(ch[..., b].any()) for b in range(len(ranges))) >= 3
    # overlapping and partial classes: counts may then sum to less or more than a partition's, each still its own range's
    W, H = 31, 17
    desc = dsrt.make_desc(W, H, 1)
    first, num = ranges[0]
    odd = [(first, num), (first, max(num // 2, 1)), (10 ** 6, 5), (-5, 5)]
    got = gpu_ctx.coverage_to_host(desc, _cd(dsrt, DIAG, 9), channels=("hits", "class_hits"), classes=dsrt.coverage_classes(odd))
    c = got["class_hits"]
    _same(c[..., 0], ch[..., 0].astype(np.uint8), "a class given twice counts the same")
    assert (c[..., 1] <= c[..., 0]).all() and not c[..., 2].any() and not c[..., 3].any()


# ---- 4. the calls ----
def test_channel_subsets_sun_disabled_all_miss_and_the_beauty_render_unchanged(dsrt, gpu_ctx):
    W, H = 40, 24
    hs, scene = _scene(dsrt, "station_near", W, H)
    gpu_ctx.upload(scene)
    desc = dsrt.make_desc(W, H, 4)
    before = gpu_ctx.render_to_host(desc, want_f32=True)
    cd = _cd(dsrt, GRID, 4)
    full = gpu_ctx.coverage_to_host(desc, cd, rep=True)
    assert full["sun_hits"].any() and (full["hits"] == 16).any() and ((full["hits"] > 0) & (full["hits"] < 16)).any()
    _same(full["alpha"], (full["hits"].astype(F) / F(16)).astype(F), "alpha is hits / n")
    _same(np.array([bin(int(m)).count("1") for m in full["mask"].ravel()], np.uint8).reshape(H, W), full["hits"], "popcount(mask) is hits")
    assert ((full["sun_mask"] & ~full["mask"]) == 0).all()
    for chans, rep in ((("mask", "sun_mask"), ()), ((), ("range", "normal")), (("hits",), ("flags",)), (("alpha",), ()), ((), ("prim_id",)), (("sun_alpha",), ("t",))):
        got = gpu_ctx.coverage_to_host(desc, cd, channels=chans, rep=rep)
        _same_coverage(got, full, ("subset", chans, rep), keys=chans, rep=rep)
    # the sun disabled: every sun output is 0, the rest unchanged
    view = hs.view(scene.camera, SUN)
    view.sun_enabled = 0
    gpu_ctx.upload(view)
    off = gpu_ctx.coverage_to_host(desc, cd, rep=True)
    assert not off["sun_hits"].any() and not off["sun_alpha"].view(np.uint32).any() and not off["sun_mask"].any() and not off["rep"]["sun_cos"].view(np.uint32).any()
    assert not (off["rep"]["flags"] & 8).any()
    _same_coverage(off, full, "sun disabled", keys=("hits", "alpha", "mask"), rep=tuple(k for k in M.GB_KEYS if k not in ("sun_cos", "flags")))
    # a camera that looks away: everything is the miss record
    away = hs.view(dsrt.camera_look_at((12.0, 9.0, 38.0), (24.0, 18.0, 76.0), 40.0, W, H, 4, 50), SUN)
    gpu_ctx.upload(away)
    miss = gpu_ctx.coverage_to_host(desc, _cd(dsrt, DIAG, 64), rep=True)
    assert not miss["hits"].any() and not miss["mask"].any() and not miss["alpha"].view(np.uint32).any()
    want = M.miss_record(H, W)
    for k in M.GB_KEYS:
        _same(miss["rep"][k], want[k], ("all miss", k))
    gpu_ctx.upload(scene)
    gpu_ctx.coverage_to_host(desc, cd)
    after = gpu_ctx.render_to_host(desc, want_f32=True)
    assert before[0].any()
    _same(after[0], before[0], "rgb8 of a render after the coverage calls"); _same(after[1], before[1], "f32 of a render after the coverage calls")


def test_device_tensors_on_a_stream(dsrt, gpu_ctx):
    W, H = 61, 35
    hs, scene = _scene(dsrt, "station_near", W, H)
    gpu_ctx.upload(scene)
    desc = dsrt.make_desc(W, H, 1)
    cd = _cd(dsrt, DIAG, 16)
    want = gpu_ctx.coverage_to_host(desc, cd, rep=True)
    side = torch.cuda.Stream(device=DEV)
    own = {"hits": torch.full((H, W), 77, dtype=torch.uint8, device=DEV), "alpha": torch.full((H, W), -1.0, device=DEV),
           "mask": torch.full((H, W), -1, dtype=torch.int64, device=DEV), "sun_hits": torch.full((H, W), 77, dtype=torch.uint8, device=DEV),
           "sun_alpha": torch.full((H, W), -1.0, device=DEV), "sun_mask": torch.full((H, W), -1, dtype=torch.int64, device=DEV)}
    rep = {}
    for k, (dt, comps) in dsrt.capi.GBUFFER_CHANNELS.items():
        tdt = {"<f4": torch.float32, "<i4": torch.int32, "u1": torch.uint8}[dt]
        rep[k] = torch.full((H, W, comps) if comps > 1 else (H, W), 5, dtype=tdt, device=DEV)
    torch.cuda.synchronize()
    assert gpu_ctx.render_coverage(desc, cd, {k: t.data_ptr() for k, t in own.items()}, {k: t.data_ptr() for k, t in rep.items()}, stream=side.cuda_stream) is None
    st = gpu_ctx.render_coverage(desc, cd, {"hits": own["hits"].data_ptr()}, stream=side.cuda_stream, want_stats=True)
    assert st.kernel_ms > 0 and st.device_flags == 0 and st.waves_launched == (W * H + 3) // 4
    side.synchronize()
    for k in OWN:
        a = own[k].cpu().numpy()
        _same(a.view(np.uint64) if k.endswith("mask") else a, want[k], ("device", k))
    for k in M.GB_KEYS:
        _same(rep[k], want["rep"][k], ("device rep", k))


def test_refusals_touch_no_buffer(dsrt, gpu_ctx):
    capi, lib = dsrt.capi, dsrt.lib
    W, H = 16, 10
    hs, scene = _scene(dsrt, "station_near", W, H)
    gpu_ctx.upload(scene)
    good = dsrt.make_desc(W, H, 1)
    hits = torch.full((H * W + 8,), 9, dtype=torch.uint8, device=DEV)
    alpha = torch.full((H * W + 2,), 9.0, device=DEV)
    mask = torch.full((H * W + 2,), 9, dtype=torch.int64, device=DEV)
    cls = torch.full((H * W * 16,), 9, dtype=torch.uint8, device=DEV)
    ptr = lambda t, off=0: C.c_void_p(t.data_ptr() + off)                     # noqa: E731

    def call(ctx=gpu_ctx._h, desc=good, cd=dsrt.coverage_desc("grid", 2), classes=None, cov="hits", host=False):
        c = capi.DsrtCoverage()
        if cov == "hits":
            c.hits = ptr(hits)
        elif cov == "misaligned alpha":
            c.alpha = ptr(alpha, 2)
        elif cov == "misaligned mask":
            c.mask = ptr(mask, 4)
        elif cov == "misaligned rep":
            c.hits = ptr(hits); c.rep.prim_id = ptr(alpha, 1)
        elif cov == "class_hits":
            c.hits = ptr(hits); c.class_hits = ptr(cls)
        ref = lambda x: C.byref(x) if x is not None else None                    # noqa: E731
        cov_p = None if cov is None else C.byref(c)
        if host:
            return lib.dsrt_render_coverage_to_host(ctx, ref(desc), ref(cd), ref(classes), cov_p, None)
        return lib.dsrt_render_coverage(ctx, ref(desc), ref(cd), ref(classes), cov_p, None, None)

    def classes(count, num0=3):
        cl = capi.DsrtCoverageClasses()
        cl.count = count
        cl.num[0] = num0
        return cl

    cases = {
        "NULL ctx": call(ctx=None), "NULL desc": call(desc=None), "NULL cov_desc": call(cd=None), "NULL cov": call(cov=None), "no output": call(cov="none"),
        "width 1": call(desc=dsrt.make_desc(1, H, 1)), "height 1": call(desc=dsrt.make_desc(W, 1, 1)), "shards": call(desc=dsrt.make_desc(W, H, 1, shard_count=2)),
        "pattern 2": call(cd=capi.DsrtCoverageDesc(2, 4)), "pattern -1": call(cd=capi.DsrtCoverageDesc(-1, 4)),
        "grid 0": call(cd=capi.DsrtCoverageDesc(0, 0)), "grid 9": call(cd=capi.DsrtCoverageDesc(0, 9)),
        "diag 0": call(cd=capi.DsrtCoverageDesc(1, 0)), "diag 65": call(cd=capi.DsrtCoverageDesc(1, 65)),
        "misaligned alpha": call(cov="misaligned alpha"), "misaligned mask": call(cov="misaligned mask"), "misaligned rep": call(cov="misaligned rep"),
        "count 17": call(classes=classes(17)), "count -1": call(classes=classes(-1)), "negative num": call(classes=classes(1, -1), cov="class_hits"),
        "class_hits without classes": call(cov="class_hits"), "class_hits with no class": call(classes=classes(0), cov="class_hits"),
        "host form: grid 9": call(cd=capi.DsrtCoverageDesc(0, 9), host=True), "host form: no output": call(cov="none", host=True),
    }
    assert {k: v for k, v in cases.items() if v != -1} == {}
    torch.cuda.synchronize()
    assert (hits == 9).all() and (alpha == 9.0).all() and (mask == 9).all() and (cls == 9).all()
    fresh = dsrt.Context(0)
    try:
        assert call(ctx=fresh._h) == -6 and call(ctx=fresh._h, host=True) == -6
    finally:
        fresh.close()
    assert call() == 0                                                    # and the call the cases vary is a good one
    torch.cuda.synchronize()
    assert (hits[:H * W] <= 4).all() and (hits[H * W:] == 9).all()


# ---- 5. the coverage-aware denoiser ----
def _dev64(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).reshape(-1).view(np.int64)).to(DEV)


def _dev_guides(g):
    return {k: torch.from_numpy(np.ascontiguousarray(g[k], np.float32)).to(DEV) for k in GUIDES}


def _desc(dsrt, W, H, spp=16, depth=50, **kw):
    return dsrt.make_desc(W, H, spp, depth, seed=SEED, rng_mode=1, **kw)


def _check_against_the_model(dsrt, ctx, oracle, what, W, H, spp, S_, S2, gh, alpha, alpha_min, gamma=2.0):
    dS, dS2, dg = _dev64(S_), _dev64(S2), _dev_guides(gh)
    da = torch.from_numpy(np.ascontiguousarray(alpha, np.float32)).to(DEV)
    for it in (0, 5):
        p = dsrt.denoise_defaults(iterations=it)
        want_c, want_v = M.denoise_coverage(S_, S2, spp, gh, alpha, alpha_min, **{**DEFAULTS, "iterations": it})
        m_rgb, m_f32 = tone_map(want_c, gamma, oracle)
        for mode in (0, 1):
            rgb, f32, lin, var = ctx.denoise_accumulated_coverage(_desc(dsrt, W, H, spp, math_mode=mode), dS, dS2, dg, da, alpha_min, samples_done=spp, params=p,
                                                                  want_f32=True, want_var=True)
            torch.cuda.synchronize()
            _same(lin, want_c, (what, it, mode, "linear")); _same(var, want_v, (what, it, mode, "var"))
            if mode == 0:
                _same(rgb, m_rgb, (what, it, "rgb8")); _same(f32, m_f32, (what, it, "f32"))
            else:                                                        # both pows are within 2 ulp of the true one: one 8-bit level at the most
                assert int(np.abs(rgb.cpu().numpy().astype(np.int16) - m_rgb.astype(np.int16)).max()) <= 1, (what, it)
    return want_c


def test_demodulated_filter_equals_the_model_on_synthetic_frames(dsrt, gpu_ctx, oracle):
    rng = np.random.default_rng(31)
    for W, H in ((37, 29), (64, 48), (3, 7)):
        S_, S2, n, g, _ = synthetic_frame(rng, W, H, spp=8, miss=0.1)
        alpha = rng.choice(np.array([0.0, 1 / 64, 1 / 16, 3 / 32, 0.25, 0.5, 63 / 64, 1.0, np.nan], F), size=(H, W)).astype(F)
        c = _check_against_the_model(dsrt, gpu_ctx, oracle, (W, H), W, H, 8, S_, S2, g, alpha, 1 / 16)
        assert np.isfinite(c).all()


def test_demodulated_filter_equals_the_model_on_a_rendered_scene_and_the_two_identities(dsrt, gpu_ctx, oracle):
    hs, scene, W, H, spp, depth = parity_case(dsrt, "station_near", SEED)
    gpu_ctx.upload(scene)
    desc = _desc(dsrt, W, H, spp, depth)
    acc = dsrt.Accumulator(gpu_ctx, desc, moments=True)
    acc.render(0)
    alpha, g = acc.coverage()
    torch.cuda.synchronize()
    S_, S2 = acc.sum.cpu().numpy().view(np.uint64).reshape(H, W, 3), acc.sum_sq.cpu().numpy().view(np.uint64).reshape(H, W, 3)
    gh, ah = {k: x.cpu().numpy() for k, x in g.items()}, alpha.cpu().numpy()
    assert ((ah > 0) & (ah < 1)).sum() > 100
    _check_against_the_model(dsrt, gpu_ctx, oracle, "station_near", W, H, spp, S_, S2, gh, ah, dsrt.coverage_alpha_min(), scene.params.gamma)
    # alpha NULL and alpha == 1 everywhere are dsrt_denoise_accumulated, byte for byte
    gb = acc.guides()
    p = dsrt.denoise_defaults()
    want = gpu_ctx.denoise_accumulated(desc, acc.sum, acc.sum_sq, gb, samples_done=spp, params=p, want_f32=True, want_var=True)
    ones = torch.ones((H, W), device=DEV)
    for a, what in ((None, "alpha NULL"), (ones, "alpha 1")):
        for amin in (1.0, 1 / 64):
            got = gpu_ctx.denoise_accumulated_coverage(desc, acc.sum, acc.sum_sq, gb, a, amin, samples_done=spp, params=p, want_f32=True, want_var=True)
            torch.cuda.synchronize()
            for x, w, k in zip(got, want, ("rgb8", "f32", "linear", "var")):
                _same(x, w, (what, amin, k))
    # the convenience form, Accumulator.denoise(alpha=True) and the host form are the same three calls
    p4 = dsrt.denoise_defaults(iterations=4)
    want = gpu_ctx.denoise_accumulated_coverage(desc, acc.sum, acc.sum_sq, g, alpha, samples_done=spp, params=p4, want_f32=True, want_var=True)
    torch.cuda.synchronize()
    rgb, f32, lin, var, a_out, st = gpu_ctx.render_denoised_coverage_to_host(desc, params=p4, want_f32=True, want_var=True, want_alpha=True)
    for x, w, k in zip((rgb, f32, lin, var), want, ("rgb8", "f32", "linear", "var")):
        _same(x, w, ("convenience", k))
    _same(a_out, ah, "the convenience form's alpha")
    assert st.kernel_ms > 0
    for x, w in zip(acc.denoise(params=p4, want_f32=True, want_var=True, alpha=True), want):
        torch.cuda.synchronize()
        _same(x, w, "Accumulator.denoise(alpha=True)")
    host = gpu_ctx.denoise_accumulated_coverage_to_host(desc, S_, S2, gh, ah, samples_done=spp, params=p4, want_f32=True, want_var=True)
    for x, w, k in zip(host, want, ("rgb8", "f32", "linear", "var")):
        _same(x, w, ("host form", k))
    # refusals: alpha_min outside (0, 1], a NaN, a GRID pattern in the convenience form -- nothing is written
    out = torch.full((H, W, 3), 7.0, device=DEV)
    gd = dsrt.capi.DsrtDenoiseGuides(**{k: C.c_void_p(g[k].data_ptr()) for k in GUIDES})
    ac = dsrt.capi.DsrtAccum(C.c_void_p(acc.sum.data_ptr()), C.c_void_p(acc.sum_sq.data_ptr()))
    for amin in (0.0, -0.5, 1.5, float("nan")):
        for a in (C.c_void_p(alpha.data_ptr()), None):
            assert dsrt.lib.dsrt_denoise_accumulated_coverage(gpu_ctx._h, C.byref(desc), C.byref(ac), spp, None, C.byref(gd), a, C.c_float(amin), C.byref(p), None, None,
                                                              C.c_void_p(out.data_ptr()), None, None) == -1
    assert dsrt.lib.dsrt_denoise_accumulated_coverage(gpu_ctx._h, C.byref(desc), C.byref(ac), spp, None, C.byref(gd), C.c_void_p(alpha.data_ptr() + 2), C.c_float(0.5),
                                                      C.byref(p), None, None, C.c_void_p(out.data_ptr()), None, None) == -1
    assert dsrt.lib.dsrt_denoise_accumulated_coverage(gpu_ctx._h, C.byref(desc), C.byref(ac), spp, None, C.byref(gd), C.c_void_p(out.data_ptr()), C.c_float(0.5),
                                                      C.byref(p), None, None, C.c_void_p(out.data_ptr()), None, None) == -1      # the output over alpha
    hout = np.zeros((H, W, 3), np.uint8)
    grid = dsrt.coverage_desc("grid", 4)
    assert dsrt.lib.dsrt_render_denoised_coverage_to_host(gpu_ctx._h, C.byref(desc), C.byref(grid), C.c_float(0.5), C.byref(p), C.c_void_p(hout.ctypes.data), None, None,
                                                          None, None, None) == -1
    torch.cuda.synchronize()
    assert (out == 7.0).all() and not hout.any()


# ---- 6. the CLI ----
def _read_ppm(path):
    data = open(path, "rb").read()
    parts = data.split(b"\n", 3)
    w, h = map(int, parts[1].split())
    return np.frombuffer(parts[3], np.uint8).reshape(h, w, 3)


def _read_pfm1(path):
    data = open(path, "rb").read()
    head, dims, scale, rest = data.split(b"\n", 3)
    assert head == b"Pf"
    w, h = map(int, dims.split())
    return np.frombuffer(rest, "<f4").reshape(h, w)[::-1]


def test_cli_coverage_and_coverage_aware_denoise(dsrt, gpu_ctx, tmp_path):
    exe = os.path.join(ROOT, "deep-space-ray-tracer_amd", "dsrt_render")
    obj = os.path.join(ASSETS, "station_3k.obj")
    poses_txt = os.path.join(GOLDEN, "rendezvous_1s_dt0_01s.txt")
    W, H, spp, it = 64, 48, 16, 3
    cmd = [exe, "--obj", obj, "--input_txt", poses_txt, "--width", str(W), "--height", str(H), "--spp", str(spp), "--frame", "98", "--frames", "1", "--rng-mode", "1",
           "--output_dir", str(tmp_path), "--denoise", str(it), "--coverage-aware", "0.125", "--coverage", "diag:16"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    hs = dsrt.HostScene().add_obj(obj)
    hs.build_bvh()
    fr = dsrt.pose_to_frame(dsrt.read_pose_file(poses_txt)[98])
    gpu_ctx.upload(hs.view(dsrt.frame_camera(fr, 40.0, W, H, spp, 50), tuple(fr.sun_dir_model)))
    desc = dsrt.make_desc(W, H, spp, 50, gamma=2.0, seed=1337, rng_mode=1)
    rgb, _, _, _, _, _ = gpu_ctx.render_denoised_coverage_to_host(desc, alpha_min=0.125, params=dsrt.denoise_defaults(iterations=it))
    plain, _, _, _, _ = gpu_ctx.render_denoised_to_host(desc, params=dsrt.denoise_defaults(iterations=it))
    assert rgb.any() and (rgb != plain).any()
    _same(_read_ppm(tmp_path / "frame_0098.ppm"), rgb, "the coverage-aware frame")
    cov = gpu_ctx.coverage_to_host(desc, dsrt.coverage_desc("diag:16"), channels=("alpha", "sun_alpha"))
    assert ((cov["alpha"] > 0) & (cov["alpha"] < 1)).any()
    _same(_read_pfm1(tmp_path / "frame_0098_alpha.pfm"), cov["alpha"], "alpha"); _same(_read_pfm1(tmp_path / "frame_0098_sun_alpha.pfm"), cov["sun_alpha"], "sun_alpha")
    assert "coverage-aware: alpha_min 0.125" in r.stdout and not (tmp_path / "frame_0098_body_alpha.pfm").exists()
    # in rng_mode 0, with a body: one plane per body, the static part first
    out2 = tmp_path / "bodies"
    cmd = [exe, "--obj", obj, "--body", obj, "--body-scale", "0.25", "--input_txt", poses_txt, "--width", str(W), "--height", str(H), "--spp", "2", "--frame", "98",
           "--frames", "1", "--output_dir", str(out2), "--coverage", "grid:3"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    a, planes = _read_pfm1(out2 / "frame_0098_alpha.pfm"), _read_pfm1(out2 / "frame_0098_body_alpha.pfm")
    assert planes.shape == (2 * H, W) and planes.any() and ((a > 0) & (a < 1)).any()
    assert np.abs((planes[:H] + planes[H:]) - a).max() < 1e-6             # ninths add up to ninths
