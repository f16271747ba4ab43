"""Temporal accumulation with bodies on the GPU (include/dsrt.h, TEMPORAL ACCUMULATION WITH BODIES; csrc/temporal_kernel.hip, dsrt_temporal_bodies_kernel) against
the numpy model of tests/_motion_model.py, bit for bit: synthetic frames over four body ranges, the reduction to the static stage, the three-frame chain of the
bodies scene posed on the device, the sequence the context keeps once it follows the bodies, refusals and stream order on a live context, and the CLI.  Every float
comparison is on uint32 views."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _bodies_model as B
import _motion_model as model
from _denoise_model import DEFAULTS as DN, F, tone_map
from _sample_sets import parity_case
from _temporal_model import random_history, wall_frame
from conftest import ASSETS, GOLDEN, ROOT
from test_temporal_bodies_host import H as CH, SEED, SPP, DEPTH, W as CW, all_poses, camera, pose_set

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUIDES = ("normal", "position", "albedo", "range")
OUTPUTS = ("rgb8", "f32", "linear", "var", "prev_xy", "weight", "prev_position")
WANT_ALL = dict(want_f32=True, want_var=True, want_prev_xy=True, want_weight=True, want_prev_position=True)


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


def _dev64(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).reshape(-1).view(np.int64)).to(DEV)


def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


def _check_frame(oracle, got, nxt, want, what, gamma=2.0):
    """got: the library's (rgb8, f32, linear, var, prev_xy, weight, prev_position), nxt its next history; want: the model's dict."""
    rgb8, f32, lin, var, pxy, wgt, ppos = got
    _same(lin, want["linear"], (what, "linear")); _same(var, want["var"], (what, "var"))
    _same(np.asarray(_bits(nxt)).reshape(want["next"].shape), want["next"], (what, "next"))
    _same(pxy, want["prev_xy"], (what, "prev_xy")); _same(wgt, want["weight"], (what, "weight")); _same(ppos, want["prev_position"], (what, "prev_position"))
    m_rgb, m_f32 = tone_map(want["linear"], gamma, oracle)
    _same(rgb8, m_rgb, (what, "rgb8")); _same(f32, m_f32, (what, "f32"))


# ---- 1. synthetic frames: no scene ----
def _synthetic(dsrt, rng, W, H):
    """The wall seen from two nearby cameras, a random prim_id image over four body ranges with every special value, and two sets of poses: bodies 1 and 3 move IN
    the wall's plane (a turn about its normal and a shift along it: their history stays valid and blends), body 2 does not move, and with `tumble` body 3 takes a
    random rotation in space instead (its points leave the wall: every tap is rejected)."""
    look = lambda p: dsrt.camera_look_at(p, (0, 0, 0), 40.0, W, H, 8, 5)              # noqa: E731
    cam1, cam0 = look((0.0, 0.0, 10.2)), look((0.3, -0.2, 10.0))
    S, S2, n, g = wall_frame(rng, cam1, W, H, miss=0.15)
    prev, _ = random_history(rng, wall_frame(rng, cam0, W, H)[3], special=0.2)
    first, num = np.array([0, 40, 100, 131], np.int32), np.array([40, 50, 31, 19], np.int32)
    edges = np.array([-1, -2, -7, 0, 39, 40, 89, 90, 99, 100, 130, 131, 149, 150, 151, 10 ** 6, 2 ** 31 - 1, -2 ** 31])
    prim = rng.integers(-4, 156, size=(H, W))
    flat = prim.reshape(-1)
    at = rng.choice(flat.size, size=min(flat.size // 8, 4 * len(edges)), replace=False)
    flat[at] = np.resize(edges, at.size)
    prim = prim.astype(np.int32)
    z = (0.0, 0.0, 1.0)
    in_plane = lambda: B._pose(B._rot(z, rng.uniform(-0.08, 0.08)), (rng.uniform(-0.4, 0.4), rng.uniform(-0.4, 0.4), 0.0))     # noqa: E731
    pp, pc = np.zeros((4, 12), F), np.zeros((4, 12), F)
    for b in (1, 2, 3):
        pp[b], pc[b] = in_plane(), in_plane()
    pc[2] = pp[2]
    tumble_p, tumble_c = pp.copy(), pc.copy()
    tumble_c[3] = B._pose(B._rot(rng.standard_normal(3), rng.uniform(0.5, 3.0)), rng.uniform(-3, 3, 3))
    n2 = n.copy(); n2[0] = 1; n2[H // 2, ::2] = 3
    return dict(S=S, S2=S2, n=n, n2=n2, g=g, cam0=cam0, prev=prev, first=first, num=num, prim=prim, poses={"in the plane": (pp, pc), "body 3 tumbles": (tumble_p, tumble_c)})


@pytest.mark.parametrize("W, H", [(33, 17), (64, 48)])
def test_synthetic_frames_equal_the_model(dsrt, gpu_ctx, oracle, W, H):
    rng = np.random.default_rng(1000 * W + H)
    s = _synthetic(dsrt, rng, W, H)
    desc = _desc(dsrt, W, H)
    body = model.body_of(s["prim"], s["first"], s["num"])
    assert all((body == b).sum() > W * H // 12 for b in range(4))
    dS, dS2, dg, dprev, dprim = _dev64(s["S"]), _dev64(s["S2"]), {k: _dev(s["g"][k]) for k in GUIDES}, _dev(s["prev"]).reshape(-1), _dev(s["prim"], np.int32)
    blended_moved = 0
    for kind, (pp, pc) in s["poses"].items():
        mo = (s["first"], s["num"], pp, pc, s["prim"])
        for counts in (None, s["n2"]):                                             # without and with d_n
            for cam, prev in ((s["cam0"], s["prev"]), (None, None)):               # ... and the first frame of a sequence: the motion still gives prev_position
                it = 2 if cam is not None else 0
                kw = dict(samples_done=8) if counts is None else dict(n=counts)
                want = model.denoise_temporal_bodies(s["S"], s["S2"], 8 if counts is None else counts, s["g"], mo, cam, prev, **{**DN, "iterations": it})
                host = gpu_ctx.denoise_temporal_bodies_to_host(desc, s["S"], s["S2"], s["g"], mo, cam, prev, params=dsrt.denoise_defaults(iterations=it), want_f32=True,
                                                               want_var=True, **kw)
                _check_frame(oracle, host[:7], host[7], want, (W, H, kind, "host form", counts is not None, cam is not None))
                nxt = torch.full((W * H * 16,), -7.5, dtype=torch.float32, device=DEV)
                dkw = dict(samples_done=8) if counts is None else dict(n=_dev(counts.astype(np.int32), np.int32))
                got = gpu_ctx.denoise_temporal_bodies(desc, dS, dS2, dg, (*mo[:4], dprim), nxt, cam, dprev if cam is not None else None,
                                                      params=dsrt.denoise_defaults(iterations=it), **WANT_ALL, **dkw)
                torch.cuda.synchronize()
                _check_frame(oracle, got, nxt, want, (W, H, kind, "device form", counts is not None, cam is not None))
                if cam is None:
                    assert (_bits(want["prev_xy"]) == 0x7FC00000).all() and not want["found"].any()
                    moved = model.moved_bodies(pp, pc)[body] & (s["g"]["range"] <= 3e38)
                    assert (_bits(want["prev_position"])[moved] != _bits(s["g"]["position"])[moved]).any(axis=1).all()
                elif counts is None:
                    moved = model.moved_bodies(pp, pc)[body]
                    blended_moved += int((want["found"] & moved).sum())
                    miss = ~(s["g"]["range"] <= 3e38)
                    assert miss.any() and not _bits(want["prev_position"])[miss].any()
                    if kind == "body 3 tumbles":
                        assert not want["found"][body == 3].any() and want["found"][body == 1].any()
    assert blended_moved > W * H // 8, "next to no pixel of a moved body blends with its history"


def test_equal_poses_reduce_to_the_static_stage(dsrt, gpu_ctx):
    W, H = 37, 29
    rng = np.random.default_rng(5)
    s = _synthetic(dsrt, rng, W, H)
    desc = _desc(dsrt, W, H)
    pc = s["poses"]["body 3 tumbles"][1]
    dS, dS2, dg, dprev, dprim = _dev64(s["S"]), _dev64(s["S2"]), {k: _dev(s["g"][k]) for k in GUIDES}, _dev(s["prev"]).reshape(-1), _dev(s["prim"], np.int32)
    nxt_b, nxt_s = (torch.zeros(W * H * 16, dtype=torch.float32, device=DEV) for _ in range(2))
    p = dsrt.denoise_defaults(iterations=3)
    got = gpu_ctx.denoise_temporal_bodies(desc, dS, dS2, dg, (s["first"], s["num"], pc, pc, dprim), nxt_b, s["cam0"], dprev, samples_done=8, params=p, **WANT_ALL)
    static = gpu_ctx.denoise_temporal(desc, dS, dS2, dg, nxt_s, s["cam0"], dprev, samples_done=8, params=p, want_f32=True, want_var=True, want_prev_xy=True, want_weight=True)
    torch.cuda.synchronize()
    for a, b, what in zip(got[:6], static, OUTPUTS):
        _same(a, b, ("all poses equal against dsrt_denoise_temporal", what))
    _same(nxt_b, nxt_s, "next")
    hit = s["g"]["range"] <= 3e38
    _same(got[6], np.where(hit[..., None], s["g"]["position"], F(0)), "prev_position is the position")
    assert bool((static[5] > 8).any())


# ---- 2. the bodies scene: Q0 -> Q1 -> Q2, posed on the device ----
def _render_frame(dsrt, ctx, k):
    """Frame k on ctx (the scene uploaded with its bodies): poses, camera, the frame's sums, its guides and prim_id from the GPU."""
    cam = camera(dsrt, k)
    ctx.set_body_poses(1, pose_set(k))
    ctx.set_camera_sun(cam, B.SUN)
    desc = _desc(dsrt, CW, CH, SPP, DEPTH, seed=SEED + k)
    acc = dsrt.Accumulator(ctx, desc, moments=True)
    acc.render(0)
    g = acc.guides()
    prim = torch.empty((CH, CW), dtype=torch.int32, device=DEV)
    ctx.render_gbuffer(desc, {"prim_id": prim.data_ptr()}, stream=ctx._raw_stream(None))
    return desc, cam, acc, g, prim


@pytest.fixture(scope="module")
def scene_chain(dsrt):
    """The explicit chain of three dsrt_denoise_temporal_bodies calls on a context of its own: per frame the library's outputs and what they were computed from."""
    ctx = dsrt.Context(0)
    try:
        hs = B.build_scene(dsrt)
        first, num = (np.array(x, np.int32) for x in zip(*[hs.body_range(b) for b in range(4)]))
        ctx.upload_bodies(hs, hs.view(camera(dsrt, 0), B.SUN))
        hist = [torch.zeros(CW * CH * 16, dtype=torch.float32, device=DEV) for _ in range(2)]
        p = dsrt.denoise_defaults(iterations=2)
        frames = []
        prev_cam = prev_poses = None
        for k in range(3):
            desc, cam, acc, g, prim = _render_frame(dsrt, ctx, k)
            poses = all_poses(k)
            mo = (first, num, poses if prev_poses is None else prev_poses, poses, prim)
            out = ctx.denoise_temporal_bodies(desc, acc.sum, acc.sum_sq, g, mo, hist[k & 1], prev_cam, hist[(k & 1) ^ 1] if k else None, samples_done=SPP, params=p, **WANT_ALL)
            torch.cuda.synchronize()
            frames.append(dict(desc=desc, cam=cam, poses=poses, prev_poses=mo[2], out=[o.cpu().numpy() for o in out], next=hist[k & 1].cpu().numpy().reshape(CH, CW, 16),
                               S=acc.sum.cpu().numpy().view(np.uint64).reshape(CH, CW, 3), S2=acc.sum_sq.cpu().numpy().view(np.uint64).reshape(CH, CW, 3),
                               g={n: x.cpu().numpy() for n, x in g.items()}, prim=prim.cpu().numpy()))
            prev_cam, prev_poses = cam, poses
        yield dict(frames=frames, first=first, num=num, params=p, hs=hs)
    finally:
        ctx.close()


def test_scene_chain_equals_the_model(dsrt, oracle, scene_chain):
    first, num = scene_chain["first"], scene_chain["num"]
    prev = prev_cam = None
    found_moved = 0
    for k, fr in enumerate(scene_chain["frames"]):
        mo = (first, num, fr["prev_poses"], fr["poses"], fr["prim"])
        want = model.denoise_temporal_bodies(fr["S"], fr["S2"], SPP, fr["g"], mo, prev_cam, prev, **{**DN, "iterations": 2})
        _check_frame(oracle, fr["out"], fr["next"], want, ("bodies scene", k))
        body = model.body_of(fr["prim"], first, num)
        found_moved += int((want["found"] & (body >= 1)).sum()) if k else 0
        prev, prev_cam = want["next"], fr["cam"]
    assert sum(int((body == b).any()) for b in (1, 2, 3)) >= 2, "the last frame shows fewer than two moved bodies"
    assert found_moved > 100, "the chain found next to no history on the moved bodies"


def test_convenience_form_follows_the_bodies(dsrt, scene_chain):
    """With dsrt_ctx_set_temporal_bodies a pose update no longer ends the context's sequence: three convenience calls with pose updates between them are the explicit
    chain; a clone under its own switch gives the same; with the switch off a pose update starts afresh, as it always did."""
    ctx = dsrt.Context(0)
    clone = None
    try:
        hs = scene_chain["hs"]
        ctx.upload_bodies(hs, hs.view(camera(dsrt, 0), B.SUN))
        assert not ctx.temporal_bodies and ctx.set_temporal_bodies(True).temporal_bodies
        clone = ctx.clone()
        assert not clone.temporal_bodies
        clone.set_temporal_bodies(True)
        p = scene_chain["params"]
        for k, fr in enumerate(scene_chain["frames"]):
            ctx.set_body_poses(1, pose_set(k))
            for c in (ctx, clone):
                c.set_camera_sun(fr["cam"], B.SUN)
                got = c.render_denoised_temporal_to_host(fr["desc"], params=p, want_f32=True, want_var=True, want_prev_xy=True)
                for a, b, ch in zip(got[:5], fr["out"][:5], OUTPUTS):
                    _same(a, b, ("frame", k, "clone" if c is clone else "context", ch))
                assert bool(np.isnan(got[4]).all()) == (k == 0)
        # the switch off again: the next pose update ends the sequence
        ctx.set_temporal_bodies(False)
        ctx.set_body_poses(1, pose_set(1))
        got = ctx.render_denoised_temporal_to_host(scene_chain["frames"][1]["desc"], params=p, want_prev_xy=True)
        assert np.isnan(got[4]).all()
        # ... and reset starts afresh with the switch on
        ctx.set_temporal_bodies(True)
        ctx.set_body_poses(1, pose_set(2))
        assert not np.isnan(ctx.render_denoised_temporal_to_host(scene_chain["frames"][2]["desc"], params=p, want_prev_xy=True)[4]).all()
        assert np.isnan(ctx.render_denoised_temporal_to_host(scene_chain["frames"][2]["desc"], params=p, want_prev_xy=True, reset=True)[4]).all()
    finally:
        if clone is not None:
            clone.close()
        ctx.close()


# ---- 3. refusals and stream order on a live context ----
def test_refusals_leave_buffers_alone_and_a_side_stream_keeps_order(dsrt, gpu_ctx):
    W, H = 37, 29
    rng = np.random.default_rng(78)
    s = _synthetic(dsrt, rng, W, H)
    pp, pc = (np.ascontiguousarray(x.reshape(-1)) for x in s["poses"]["in the plane"])
    first, num = s["first"], s["num"]
    desc = _desc(dsrt, W, H)
    dn, tp = dsrt.denoise_defaults(iterations=3), dsrt.temporal_defaults()
    want = model.denoise_temporal_bodies(s["S"], s["S2"], 8, s["g"], (first, num, pp, pc, s["prim"]), s["cam0"], s["prev"], **{**DN, "iterations": 3})
    assert want["found"].sum() > 200
    dS, dS2, dg, dprev, dprim = _dev64(s["S"]), _dev64(s["S2"]), {k: _dev(s["g"][k]) for k in GUIDES}, _dev(s["prev"]).reshape(-1), _dev(s["prim"], np.int32)
    inputs = [dS, dS2, dprev, dprim] + [dg[k] for k in GUIDES]
    keep = [t.clone() for t in inputs]
    sentinel = lambda dt, shape=(H, W, 3): torch.full(shape, 0x5A if dt == torch.uint8 else -7.5, dtype=dt, device=DEV)   # noqa: E731
    outs = [sentinel(torch.uint8), sentinel(torch.float32), sentinel(torch.float32), sentinel(torch.float32)]
    nxt, pxy, wgt, ppos = sentinel(torch.float32, (H * W * 16,)), sentinel(torch.float32, (H, W, 2)), sentinel(torch.float32, (H, W)), sentinel(torch.float32, (H * W * 3 + 1,))
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None              # noqa: E731
    hptr = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None            # noqa: E731

    def changed(a, i, v):
        b = a.copy()
        b[i] = v
        return b

    def call(bodies=4, first=first, num=num, pp=pp, pc=pc, prim=dprim, cam=s["cam0"], prev=dprev, nxt=nxt, outs=outs, pxy=pxy, wgt=wgt, ppos=ppos[:H * W * 3], null_motion=False):
        acc = dsrt.capi.DsrtAccum(ptr(dS), ptr(dS2))
        gd = dsrt.capi.DsrtDenoiseGuides(*[ptr(dg[k]) for k in GUIDES])
        m = dsrt.capi.DsrtBodyMotion(bodies, hptr(first), hptr(num), hptr(pp), hptr(pc), ptr(prim))
        return dsrt.lib.dsrt_denoise_temporal_bodies(gpu_ctx._h, C.byref(desc), C.byref(acc), 8, None, C.byref(gd), None if null_motion else C.byref(m),
                                                     C.byref(cam) if cam is not None else None, ptr(prev), ptr(nxt), C.byref(tp), C.byref(dn), *[ptr(o) for o in outs], ptr(pxy),
                                                     ptr(wgt), ptr(ppos), None)

    refusals = {
        "NULL motion": call(null_motion=True), "NULL poses_cur": call(pc=None), "NULL prim_id": call(prim=None), "bodies 17": call(bodies=17), "bodies 0": call(bodies=0),
        "negative num_tris": call(num=changed(num, 1, -1)), "ranges overlap": call(first=changed(first, 3, 120)), "NaN pose": call(pp=changed(pp, 30, np.nan)),
        "camera without history": call(prev=None), "NULL next": call(nxt=None), "next is prev": call(nxt=dprev),
        "prim_id misaligned": call(prim=dprim.view(torch.int16).reshape(-1)[1:]), "linear over prim_id": call(outs=[outs[0], outs[1], dprim.view(torch.float32), outs[3]]),
        "prev_position misaligned": call(ppos=ppos.view(torch.int16)[1:]), "prev_position over an input": call(ppos=dg["normal"]), "prev_position over next": call(ppos=nxt),
        "prev_position over prev_xy": call(ppos=pxy), "prev_position over prim_id": call(ppos=dprim.view(torch.float32)),
        "first frame: NULL motion": call(cam=None, prev=None, null_motion=True), "first frame: inf pose": call(cam=None, prev=None, pc=changed(pc, 14, np.inf)),
    }
    assert {k: v for k, v in refusals.items() if v != -1} == {}
    torch.cuda.synchronize()
    assert (outs[0] == 0x5A).all() and all((o == -7.5).all() for o in outs[1:] + [nxt, pxy, wgt, ppos])
    for was, now in zip(keep, inputs):
        assert torch.equal(was.view(torch.uint8), now.view(torch.uint8))
    # the call itself: every output element written, every input untouched
    assert call() == 0
    torch.cuda.synchronize()
    _same(outs[2], want["linear"], "linear"); _same(outs[3], want["var"], "var"); _same(nxt.reshape(H, W, 16), want["next"], "next")
    _same(pxy, want["prev_xy"], "prev_xy"); _same(wgt, want["weight"], "weight"); _same(ppos[:H * W * 3].reshape(H, W, 3), want["prev_position"], "prev_position")
    assert float(ppos[-1]) == -7.5 and not (outs[1] == -7.5).any()
    for was, now in zip(keep, inputs):
        assert torch.equal(was.view(torch.uint8), now.view(torch.uint8))
    # asynchronous, on a side stream: the call is made while the work that makes its inputs is still queued there, between two renders of the same context
    hs, scene, RW, RH, rspp, rdepth = parity_case(dsrt, "textured", SEED)
    gpu_ctx.upload(scene)
    rdesc = _desc(dsrt, RW, RH, rspp, rdepth)
    ref = gpu_ctx.render_to_host(rdesc)[0]
    side = torch.cuda.Stream(device=DEV)
    hS, hS2 = (torch.from_numpy(a.reshape(-1).view(np.int64)).pin_memory() for a in (s["S"], s["S2"]))
    hprev, hprim = torch.from_numpy(s["prev"].reshape(-1)).pin_memory(), torch.from_numpy(s["prim"]).pin_memory()
    before, after = torch.zeros((RH, RW, 3), dtype=torch.uint8, device=DEV), torch.zeros((RH, RW, 3), dtype=torch.uint8, device=DEV)
    nxt2 = torch.zeros(H * W * 16, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        filler = torch.zeros(1 << 24, device=DEV)
        for _ in range(8):
            filler += 1.0                                                            # work in front of the copies, so that they are still queued when the call is made
        sS, sS2, sprev, sprim = (t.to(DEV, non_blocking=True) for t in (hS, hS2, hprev, hprim))
        sg = {k: (dg[k] * 1.0) for k in GUIDES}
        gpu_ctx.render(rdesc, before.data_ptr(), stream=side.cuda_stream)
        _, _, lin, var, spxy, swgt, sppos = gpu_ctx.denoise_temporal_bodies(desc, sS, sS2, sg, (first, num, pp, pc, sprim), nxt2, s["cam0"], sprev, samples_done=8, params=dn,
                                                                            want_rgb8=False, want_var=True, want_prev_xy=True, want_weight=True, want_prev_position=True, stream=side)
        gpu_ctx.render(rdesc, after.data_ptr(), stream=side.cuda_stream)
    side.synchronize()
    _same(lin, want["linear"], "linear, side stream"); _same(var, want["var"], "var, side stream"); _same(nxt2.reshape(H, W, 16), want["next"], "next, side stream")
    _same(spxy, want["prev_xy"], "prev_xy, side stream"); _same(swgt, want["weight"], "weight, side stream"); _same(sppos, want["prev_position"], "prev_position, side stream")
    assert ref.any()
    _same(before, ref, "the render queued before the call"); _same(after, ref, "the render queued after the call")


# ---- 4. the CLI ----
def _read_pfm(path):
    data = open(path, "rb").read()
    head, dims, scale, rest = data.split(b"\n", 3)
    assert head == b"PF"
    w, h = map(int, dims.split())
    return np.frombuffer(rest, "<f4").reshape(h, w, 3)[::-1].reshape(h, w, 3)


def test_cli_follow_bodies_and_flow(dsrt, gpu_ctx, tmp_path):
    W, H, spp, it = 48, 32, 4, 1
    exe = os.path.join(ROOT, "deep-space-ray-tracer_amd", "dsrt_render")
    obj = os.path.join(ASSETS, "station_3k.obj")
    poses_txt = os.path.join(GOLDEN, "rendezvous_1s_dt0_01s.txt")
    body_obj = tmp_path / "visitor.obj"
    v = [(x, y, z) for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)]
    quads = [(1, 2, 4, 3), (5, 7, 8, 6), (1, 5, 6, 2), (3, 4, 8, 7), (1, 3, 7, 5), (2, 6, 8, 4)]
    body_obj.write_text("".join(f"v {a} {b} {c}\n" for a, b, c in v) + "".join(f"f {a} {b} {c}\nf {a} {c} {d}\n" for a, b, c, d in quads))
    poses = dsrt.read_pose_file(poses_txt)
    frs = [dsrt.pose_to_frame(poses[i]) for i in (97, 98)]
    eye = np.array(frs[0].cam_in_model[:], np.float64)
    scale = round(0.04 * float(np.linalg.norm(eye)), 3)                                        # a visitor halfway between the camera and the station, well inside the view
    body_poses = np.stack([B._pose(B._rot((1, 2, 3), 0.5 + 0.05 * k), (0.5 + 0.01 * k) * np.array(fr.cam_in_model[:], np.float64)) for k, fr in enumerate(frs)])
    (tmp_path / "body_poses.txt").write_text("# visitor\n" + "".join(" ".join(repr(float(x)) for x in p) + "\n" for p in body_poses))
    base = [exe, "--obj", obj, "--body", str(body_obj), "--body-scale", repr(scale), "--body-poses", str(tmp_path / "body_poses.txt"), "--input_txt", poses_txt,
            "--width", str(W), "--height", str(H), "--spp", str(spp), "--frame", "97", "--frames", "2", "--rng-mode", "1", "--denoise", str(it), "--temporal", "--flow"]
    out_f, out_s = tmp_path / "follow", tmp_path / "static"
    r = subprocess.run(base + ["--follow-bodies", "--output_dir", str(out_f)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r2 = subprocess.run(base + ["--output_dir", str(out_s)], capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0, r2.stdout + r2.stderr
    # the library chain
    hs = dsrt.HostScene().add_obj(obj)
    assert hs.begin_body() == 1
    hs.add_obj(str(body_obj), scale)
    hs.build_bvh_bodies()
    first, num = (np.array(x, np.int32) for x in zip(*[hs.body_range(b) for b in range(2)]))
    p = dsrt.denoise_defaults(iterations=it)
    hist = [torch.zeros(W * H * 16, dtype=torch.float32, device=DEV) for _ in range(2)]
    ys, xs = np.mgrid[0:H, 0:W]
    prev_cam = prev_poses = None
    for k, (i, fr) in enumerate(zip((97, 98), frs)):
        cam = dsrt.frame_camera(fr, 40.0, W, H, spp, 50)
        if k == 0:
            gpu_ctx.upload_bodies(hs, hs.view(cam, tuple(fr.sun_dir_model)))
        gpu_ctx.set_body_poses(1, body_poses[k:k + 1])
        gpu_ctx.set_camera_sun(cam, tuple(fr.sun_dir_model))
        desc = dsrt.make_desc(W, H, spp, 50, gamma=2.0, seed=1337 + i, rng_mode=1)
        acc = dsrt.Accumulator(gpu_ctx, desc, moments=True)
        acc.render(0)
        prim = torch.empty((H, W), dtype=torch.int32, device=DEV)
        gpu_ctx.render_gbuffer(desc, {"prim_id": prim.data_ptr()}, stream=gpu_ctx._raw_stream(None))
        cur = np.concatenate([np.zeros((1, 12), F), body_poses[k:k + 1]]).astype(F)
        mo = (first, num, cur if prev_poses is None else prev_poses, cur, prim)
        out = gpu_ctx.denoise_temporal_bodies(desc, acc.sum, acc.sum_sq, acc.guides(), mo, hist[k], prev_cam, hist[0] if k else None, samples_done=spp, params=p, want_prev_xy=True)
        torch.cuda.synchronize()
        pxy = out[4].cpu().numpy()
        flow = np.stack([pxy[..., 0] - xs.astype(F), pxy[..., 1] - ys.astype(F), np.zeros((H, W), F)], -1).astype(F)
        got = _read_pfm(out_f / f"frame_{i:04d}_flow.pfm")
        assert np.array_equal(np.isnan(got), np.isnan(flow)) and np.array_equal(got[~np.isnan(got)].view(np.uint32), flow[~np.isnan(flow)].view(np.uint32)), (i, "flow")
        static = _read_pfm(out_s / f"frame_{i:04d}_flow.pfm")
        if k:
            on_body = prim.cpu().numpy() >= first[1]
            assert on_body.sum() > 20 and not np.isnan(flow[on_body][:, :2]).all()
            assert np.isnan(static[..., :2]).all(), "without --follow-bodies a pose update starts the history afresh: no flow"
        else:
            assert np.isnan(flow[..., :2]).all() and np.isnan(static[..., :2]).all()
        prev_cam, prev_poses = cam, cur
