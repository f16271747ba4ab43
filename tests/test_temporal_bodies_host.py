"""Temporal accumulation with bodies on the CPU (include/dsrt.h, TEMPORAL ACCUMULATION WITH BODIES): dsrt_body_motion_host against the numpy model of
tests/_motion_model.py bit for bit, everything the entry points refuse without a device, the motion rule against the geometry it stands for (the same material
point of the same triangle in the previous frame's pose, in float64), and what the stage buys on a three-frame chain of the bodies scene -- all on the oracle's
G-buffers and sums, no GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _bodies_model as B
import _motion_model as model
from _denoise_model import DEFAULTS as DN, F
from _sample_sets import SetOracle
from _temporal_model import DEFAULTS, denoise_temporal, project
from conftest import ROOT

GUIDES = ("normal", "position", "albedo", "range")
W, H, SPP, DEPTH, SEED = 64, 48, 8, 8, 0xDEADBEEF00001337


# ---- the sequence: three pose sets and three cameras ----
# Every body >= 1 is brought in front of the camera, then turns by a few degrees and shifts by about a metre per frame -- several pixels of image motion -- with a
# component along every face's normal well above plane_tol * range (0.01 * 15 m), so that the static stage cannot take a moved surface for its own history.
_REST_CENTRE = {1: (8.0, 0.0, 3.0), 2: B.PATCH_REST, 3: (-9.0, -8.0, 4.0)}
_START = {1: (1.5, -1.0, 6.0), 2: (-4.0, 1.0, 5.0), 3: (-1.0, -5.5, 7.0)}
_STEP = {1: (0.7, 0.5, 0.5), 2: (0.3, -0.8, 0.5), 3: (0.6, 0.6, 0.5)}
_AXIS = {1: (0.2, 0.3, 1.0), 2: (1.0, 0.2, 0.1), 3: (0.3, 1.0, 0.2)}
_TURN = {1: (0.4, np.radians(4.0)), 2: (0.1, np.radians(3.0)), 3: (0.7, np.radians(5.0))}                # (angle at Q0, per frame)


def pose_set(k):
    """Q_k: (3, 12) float32 for bodies 1, 2, 3 -- the rest pose turned about the body's own centre and carried to its place in frame k."""
    out = []
    for b in (1, 2, 3):
        R = B._rot(_AXIS[b], _TURN[b][0] + k * _TURN[b][1])
        at = np.array(_START[b]) + k * np.array(_STEP[b])
        out.append(B._pose(R, at - R @ np.array(_REST_CENTRE[b])))
    return np.stack(out)


def lookfrom(k):
    """The camera moves about a hundredth of its distance to the target per frame."""
    return (B.LOOKFROM[0] + 0.15 * k, B.LOOKFROM[1] + 0.1 * k, B.LOOKFROM[2] - 0.1 * k)


def camera(dsrt, k, w=W, h=H):
    return dsrt.camera_look_at(lookfrom(k), B.LOOKAT, B.VFOV, w, h, SPP, DEPTH)


def all_poses(k):
    """(4, 12): Q_k with body 0's ignored entry in front."""
    return np.concatenate([np.zeros((1, 12), F), pose_set(k)]).astype(F)


def ranges(hs):
    r = [hs.body_range(b) for b in range(4)]
    return np.array([a for a, _ in r], np.int32), np.array([n for _, n in r], np.int32)


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---- 1. ABI ----
def test_struct_size_and_exports(dsrt):
    capi = dsrt.capi
    assert dsrt.lib.dsrt_sizeof(18) == C.sizeof(capi.DsrtBodyMotion) == 8 + 5 * C.sizeof(C.c_void_p)
    assert [f for f, _ in capi.DsrtBodyMotion._fields_] == ["bodies", "first_tri", "num_tris", "poses_prev", "poses_cur", "prim_id"]
    assert capi.ABI_VERSION == dsrt.lib.dsrt_abi_version() == 8                       # additive: the version stays
    for name in ("dsrt_body_motion_host", "dsrt_denoise_temporal_bodies", "dsrt_denoise_temporal_bodies_to_host", "dsrt_ctx_set_temporal_bodies", "dsrt_ctx_temporal_bodies"):
        assert name in capi.EXPORTS and hasattr(dsrt.lib, name)
    for m in ("denoise_temporal_bodies", "denoise_temporal_bodies_to_host", "set_temporal_bodies"):
        assert hasattr(dsrt.Context, m)
    assert dsrt.lib.dsrt_ctx_temporal_bodies(None) == 0 and dsrt.lib.dsrt_ctx_set_temporal_bodies(None, 1) == -1


# ---- 2. the host form equals the model ----
def _random_motion(rng, n):
    """Four body ranges, random rotations as float32 poses, body 2 unmoved; prim_id over every special value, every range, just outside each end and beyond the last."""
    first, num = np.array([0, 40, 100, 131], np.int32), np.array([40, 50, 31, 19], np.int32)          # a gap between bodies 1 and 2; 2 and 3 touch
    pp, pc = np.zeros((4, 12), F), np.zeros((4, 12), F)
    for b in range(1, 4):
        for p in (pp, pc):
            p[b] = B._pose(B._rot(rng.standard_normal(3), rng.uniform(0, np.pi)), rng.uniform(-50, 50, 3))
    pc[2] = pp[2]
    pp[0], pc[0] = 1.0, 2.0                                                           # entry 0 is ignored: body 0 never moves
    edges = [-1, -2, -7, 0, 39, 40, 89, 90, 99, 100, 130, 131, 149, 150, 151, 10 ** 6, 2 ** 31 - 1, -2 ** 31]
    prim = np.concatenate([np.array(edges), rng.integers(-8, 160, n - len(edges))]).astype(np.int32)
    scale = 10.0 ** rng.uniform(-3, 4, (n, 1))
    X = (rng.standard_normal((n, 3)) * scale).astype(F)
    N = rng.standard_normal((n, 3))
    N = (N / np.linalg.norm(N, axis=1, keepdims=True)).astype(F)
    on2 = np.nonzero((prim >= 100) & (prim < 131))[0]
    X[on2[0], 1] = F(-0.0)                                                            # an unmoved body's point keeps its bits, a -0.0 coordinate included
    N[on2[1]] = (F(-0.0), F(0.0), F(1.0))
    return first, num, pp, pc, prim, N, X


def test_host_form_equals_the_model_bit_for_bit(dsrt):
    rng = np.random.default_rng(20241)
    first, num, pp, pc, prim, N, X = _random_motion(rng, 6000)
    body = model.body_of(prim, first, num)
    assert [int((body == b).sum()) > 500 for b in range(4)] == [True] * 4 and list(model.moved_bodies(pp, pc)) == [False, True, False, True]
    assert list(body[:18]) == [0, 0, 0, 0, 0, 1, 1, 0, 0, 2, 2, 3, 3, 0, 0, 0, 0, 0]
    wantN, wantX = model.motion(first, num, pp, pc, prim, N, X)
    gotN, gotX = dsrt.body_motion_host(first, num, pp, pc, prim, N, X)
    assert np.array_equal(_bits(gotX), _bits(wantX)) and np.array_equal(_bits(gotN), _bits(wantN))
    still = (body == 0) | (body == 2)
    assert np.array_equal(_bits(gotX)[still], _bits(X)[still]) and np.array_equal(_bits(gotN)[still], _bits(N)[still])
    assert (_bits(gotX)[~still] != _bits(X)[~still]).any(axis=1).all()
    assert (_bits(gotX) == 0x80000000).any() and (_bits(gotN) == 0x80000000).any()
    # a rigid motion: lengths and angles stay (the poses are rotations to float32 accuracy)
    mv = ~still
    assert np.abs(np.linalg.norm(gotN[mv].astype(np.float64), axis=1) - 1).max() < 1e-5
    # all poses equal: nothing moves, bit for bit
    sameN, sameX = dsrt.body_motion_host(first, num, pc, pc, prim, N, X)
    assert np.array_equal(_bits(sameX), _bits(X)) and np.array_equal(_bits(sameN), _bits(N))
    # back and forth returns to the point within the rule's rounding
    backN, backX = dsrt.body_motion_host(first, num, pc, pp, prim, gotN, gotX)
    M = max(np.abs(X).max(), 50.0)
    assert np.abs(backX.astype(np.float64) - X).max() <= 512 * 2.0 ** -24 * M


# ---- 3. refusals ----
def test_refusals_of_the_host_form(dsrt):
    capi, lib = dsrt.capi, dsrt.lib
    rng = np.random.default_rng(7)
    first, num, pp, pc, prim, N, X = _random_motion(rng, 64)
    pp, pc = pp.reshape(-1).copy(), pc.reshape(-1).copy()
    outN, outX = np.full((65, 3), -7.5, F), np.full((65, 3), -7.5, F)
    ptr = lambda a, off=0: C.c_void_p(a.ctypes.data + off) if a is not None else None   # noqa: E731

    def call(bodies=4, first=first, num=num, pp=pp, pc=pc, prim=prim, n=64, N=N, X=X, oN=outN, oX=outX, off=0, null_motion=False):
        m = capi.DsrtBodyMotion(bodies, ptr(first), ptr(num), ptr(pp), ptr(pc), ptr(prim, off))
        return lib.dsrt_body_motion_host(None if null_motion else C.byref(m), n, ptr(N), ptr(X), ptr(oN), ptr(oX))

    def changed(a, i, v):
        b = a.copy()
        b[i] = v
        return b

    cases = {
        "NULL motion": call(null_motion=True), "NULL first_tri": call(first=None), "NULL num_tris": call(num=None), "NULL poses_prev": call(pp=None),
        "NULL poses_cur": call(pc=None), "NULL prim_id": call(prim=None), "bodies 0": call(bodies=0), "bodies 17": call(bodies=17), "bodies -1": call(bodies=-1),
        "negative first_tri": call(first=changed(first, 2, -1)), "negative num_tris": call(num=changed(num, 3, -1)), "negative first_tri of body 0": call(first=changed(first, 0, -5)),
        "ranges overlap": call(first=changed(first, 2, 89)), "a range inside another": call(first=changed(first, 3, 50), num=changed(num, 3, 5)),
        "NaN in poses_cur": call(pc=changed(pc, 12 + 5, np.nan)), "inf in poses_prev": call(pp=changed(pp, 47, np.inf)),
        "n < 0": call(n=-1), "NULL normal": call(N=None), "NULL position": call(X=None), "prim_id misaligned": call(off=2),
        "output over an input": call(oX=X), "outputs overlap": call(oN=outX), "output over prim_id": call(oN=prim.view(F)),
    }
    assert {k: v for k, v in cases.items() if v != -1} == {}
    assert lib.dsrt_last_error()
    assert (outN == -7.5).all() and (outX == -7.5).all()
    # accepted: body 0's range may overlap the others' (it is not looked at), an empty range may lie anywhere, entry 0 of the poses may hold anything
    assert call(first=changed(first, 0, 45)) == 0 and call(first=changed(first, 2, 60), num=changed(num, 2, 0)) == 0
    assert call(pp=changed(pp, 3, np.nan), pc=changed(pc, 0, np.inf)) == 0
    assert call(bodies=1) == 0 and np.array_equal(_bits(outX[:64]), _bits(X)) and (outX[64] == -7.5).all()
    assert call(oN=None) == 0 and call(oX=None) == 0 and call(n=0) == 0


def test_refusals_of_the_denoiser_forms_that_need_no_device(dsrt):
    """Every argument check of dsrt_denoise_temporal_bodies comes before the context or any buffer is looked at: a stand-in for the context and host arrays do."""
    capi, lib = dsrt.capi, dsrt.lib
    w, h = 8, 6
    px = w * h
    ctx = C.cast(C.create_string_buffer(64), C.c_void_p)                            # never dereferenced: every call below is refused
    S, S2 = np.zeros(px * 3 + 1, np.uint64), np.zeros(px * 3 + 1, np.uint64)
    f32 = lambda k: np.full(px * k + 4, -7.5, np.float32)                            # noqa: E731
    N, X, A, R = f32(3), f32(3), f32(3), f32(1)
    rgb, lin, var = np.full(px * 3, 0x5A, np.uint8), f32(3), f32(3)
    hp, hn = dsrt.aligned_zeros(px * 16 + 16), dsrt.aligned_zeros(px * 16 + 16)
    hp[:], hn[:] = -7.5, -7.5
    pxy, wgt, ppos = f32(2), f32(1), f32(3)
    prim = np.full(px + 4, -1, np.int32)
    first, num = np.array([0, 10, 20], np.int32), np.array([10, 10, 10], np.int32)
    pp, pc = np.tile(B._pose(np.eye(3), (0, 0, 0)), 3), np.tile(B._pose(np.eye(3), (1, 0, 0)), 3)
    cam = dsrt.camera_look_at((0, 0, 10), (0, 0, 0), 40.0, w, h, 4, 5)
    ptr = lambda a, off=0: C.c_void_p(a.ctypes.data + off) if a is not None else None   # noqa: E731
    ref = lambda x: C.byref(x) if x is not None else None                            # noqa: E731
    good = dsrt.make_desc(w, h, 4, rng_mode=1)
    T = dsrt.temporal_defaults

    def changed(a, i, v):
        b = a.copy()
        b[i] = v
        return b

    def call(desc=good, sq=S2, done=4, guides=(N, X, A, R), cam=cam, prev=hp, nxt=hn, tp="default", dn="default", outs=(rgb, None, lin, var), pxy=pxy, wgt=wgt, ppos=ppos,
             ppos_off=0, bodies=3, first=first, num=num, pp=pp, pc=pc, prim=prim, prim_off=0, null_motion=False, fn="dev"):
        a = capi.DsrtAccum(ptr(S), ptr(sq))
        g = capi.DsrtDenoiseGuides(*[ptr(x) for x in guides])
        m = capi.DsrtBodyMotion(bodies, ptr(first), ptr(num), ptr(pp), ptr(pc), ptr(prim, prim_off))
        tp = T() if tp == "default" else tp
        dn = dsrt.denoise_defaults() if dn == "default" else dn
        args = [ctx, ref(desc), ref(a), done, None, ref(g), None if null_motion else ref(m), ref(cam), ptr(prev), ptr(nxt), ref(tp), ref(dn)] + [ptr(o) for o in outs] + \
               [ptr(pxy), ptr(wgt), ptr(ppos, ppos_off)]
        return lib.dsrt_denoise_temporal_bodies(*args, None) if fn == "dev" else lib.dsrt_denoise_temporal_bodies_to_host(*args)

    cases = {}
    for fn in ("dev", "host"):
        c = lambda **kw: call(fn=fn, **kw)                                          # noqa: E731
        cases.update({(fn, k): v for k, v in {
            # dsrt_denoise_temporal's own, one of each class
            "NULL sum_sq": c(sq=None), "NULL guide": c(guides=(N, X, None, R)), "rng_mode 0": c(desc=dsrt.make_desc(w, h, 4, rng_mode=0)), "samples_done 1": c(done=1),
            "iterations 7": c(dn=dsrt.denoise_defaults(iterations=7)), "no output": c(outs=(None,) * 4), "output over an input": c(outs=(rgb, None, N, var)),
            "camera without history": c(prev=None), "history without camera": c(cam=None), "NULL next": c(nxt=None), "NULL DsrtTemporal": c(tp=None),
            "alpha_min NaN": c(tp=T(alpha_min=float("nan"))), "plane_tol 0": c(tp=T(plane_tol=0.0)), "next is prev": c(nxt=hp), "prev_xy over weight": c(wgt=pxy),
            # the motion's
            "NULL motion": c(null_motion=True), "NULL first_tri": c(first=None), "NULL num_tris": c(num=None), "NULL poses_prev": c(pp=None), "NULL poses_cur": c(pc=None),
            "NULL prim_id": c(prim=None), "bodies 0": c(bodies=0), "bodies 17": c(bodies=17), "negative first_tri": c(first=changed(first, 1, -1)),
            "negative num_tris": c(num=changed(num, 2, -3)), "ranges overlap": c(first=changed(first, 2, 19)), "NaN pose": c(pc=changed(pc, 13, np.nan)),
            "inf pose": c(pp=changed(pp, 35, -np.inf)), "prim_id misaligned": c(prim_off=2), "linear over prim_id": c(outs=(rgb, None, prim.view(F), var)),
            "next over prim_id": c(nxt=hp, prev=hn, prim=hp.view(np.int32)), "weight over prim_id": c(wgt=prim.view(F)),
            "prev_position misaligned": c(ppos_off=1), "prev_position over an input": c(ppos=X), "prev_position over prim_id": c(ppos=prim.view(F)),
            "prev_position over an output": c(ppos=lin), "prev_position over prev": c(ppos=hp), "prev_position over next": c(ppos=hn), "prev_position over prev_xy": c(ppos=pxy),
            "first frame: NULL motion": c(cam=None, prev=None, null_motion=True), "first frame: bodies 0": c(cam=None, prev=None, bodies=0),
            "first frame: NaN pose": c(cam=None, prev=None, pp=changed(pp, 20, np.nan)),
        }.items()})
    assert {k: v for k, v in cases.items() if v != -1} == {}
    assert lib.dsrt_last_error()
    # a good motion is accepted: the call gets as far as a later refusal
    assert call(ppos_off=0, nxt=hn[1:]) == -1 and b"16-byte aligned" in lib.dsrt_last_error()
    assert (rgb == 0x5A).all() and (prim == -1).all() and all((a == -7.5).all() for a in (lin, var, hp, hn, pxy, wgt, ppos, N, X, A, R))


@pytest.mark.parametrize("flags, says", [
    (["--rng-mode", "1", "--denoise", "--temporal", "--follow-bodies"], "--follow-bodies needs --body"),
    (["--rng-mode", "1", "--denoise", "--follow-bodies", "--body", "x.obj"], "--follow-bodies needs --body, --denoise and --temporal"),
    (["--rng-mode", "1", "--temporal", "--follow-bodies", "--body", "x.obj"], "--denoise"),
])
def test_cli_usage_errors(flags, says, tmp_path):
    exe = os.path.join(ROOT, "deep-space-ray-tracer_amd", "dsrt_render")
    r = subprocess.run([exe, "--obj", "none.obj", "--output_dir", str(tmp_path)] + flags, capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and says in r.stderr, r.stderr


def test_cli_usage_names_the_flag():
    exe = os.path.join(ROOT, "deep-space-ray-tracer_amd", "dsrt_render")
    r = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
    assert "--follow-bodies" in r.stdout + r.stderr


# ---- 4. the three-frame chain Q0 -> Q1 -> Q2 of the bodies scene, on the oracle's G-buffers and sums ----
@pytest.fixture(scope="module")
def chain(dsrt, oracle):
    """[frame k: dict(hs, cam, scene, gb, S, S2, poses)] for k = 0, 1, 2, computed once."""
    from test_gpu_gbuffer import expected_gbuffer
    sets = SetOracle()
    out = []
    for k in range(3):
        hs = B.build_scene(dsrt)
        hs.set_body_poses(1, pose_set(k))
        cam = camera(dsrt, k)
        scene = hs.view(cam, B.SUN)
        scene.seed = SEED + k
        gb = expected_gbuffer(oracle, hs, scene, W, H)
        S, S2 = sets.sums(scene, W, H, 0, SPP)
        out.append(dict(hs=hs, cam=cam, scene=scene, gb=gb, S=S, S2=S2, poses=all_poses(k)))
    return out


def _guides(fr):
    return {k: fr["gb"][k] for k in GUIDES}


def test_motion_is_the_same_material_point_in_the_previous_pose(dsrt, chain):
    """For every pixel on a moved body in frame Q2: X' against the point of the SAME triangle at the SAME barycentric coordinates in the scene posed with Q1, in
    float64, and prev_xy against that point through frame Q1's camera.  The rule is about 20 roundings of intermediates of at most 3 M, each at most 2^-24 relative:
    60 * 2^-24 * M at worst; 256 leaves a factor of four.  Measured: 9.9 * 2^-24 * M (M = 9.02) over 436 pixels; prev_xy within 2.2e-5 px (bound 2e-3)."""
    prev, cur = chain[1], chain[2]
    first, num = ranges(cur["hs"])
    gb = cur["gb"]
    body = model.body_of(gb["prim_id"], first, num)
    on = body >= 1
    counts = [int((body == b).sum()) for b in (1, 2, 3)]
    assert all(c >= need for c, need in zip(counts, (60, 40, 10))), counts
    assert model.moved_bodies(prev["poses"], cur["poses"])[1:].all()
    N2, X2 = dsrt.body_motion_host(first, num, prev["poses"], cur["poses"], gb["prim_id"], gb["normal"], gb["position"])
    X2 = X2.reshape(H, W, 3)
    tris = prev["hs"].arrays()["tris"]["v"].astype(np.float64)[gb["prim_id"][on]]
    u, v = gb["uv"][on][:, 0:1].astype(np.float64), gb["uv"][on][:, 1:2].astype(np.float64)
    truth = tris[:, 0] + u * (tris[:, 1] - tris[:, 0]) + v * (tris[:, 2] - tris[:, 0])
    M = max(np.abs(gb["position"][on]).max(), np.abs(truth).max(), np.abs(prev["poses"][1:, 3::4]).max(), np.abs(cur["poses"][1:, 3::4]).max())
    worst = np.abs(X2[on].astype(np.float64) - truth).max()
    print(f"max |X' - X_true| = {worst:.3e} = {worst / (2.0 ** -24 * M):.1f} * 2^-24 * M, M = {M:.2f}, over {int(on.sum())} pixels")
    assert worst <= 256 * 2.0 ** -24 * M
    # the flow: prev_xy of the stage against the float64 projection of the true point through the previous camera
    res = model.denoise_temporal_bodies(cur["S"], cur["S2"], SPP, _guides(cur), (first, num, prev["poses"], cur["poses"], gb["prim_id"]), prev["cam"],
                                        np.zeros((H, W, 16), F), iterations=0)
    from _temporal_model import camera_vectors
    Cm = {k: x.astype(np.float64) for k, x in camera_vectors(prev["cam"]).items()}
    D = truth - Cm["origin"]
    e = Cm["lower_left_corner"] - Cm["origin"]
    k = (e @ Cm["w"]) / (D @ Cm["w"])
    s, t = ((D @ Cm["u"]) * k - e @ Cm["u"]) / (Cm["horizontal"] @ Cm["u"]), ((D @ Cm["v"]) * k - e @ Cm["v"]) / (Cm["vertical"] @ Cm["v"])
    want = np.stack([s * (W - 1) - 0.5, (H - 1) - (t * (H - 1) - 0.5)], -1)
    got = res["prev_xy"][on].astype(np.float64)
    seen = ~np.isnan(got[:, 0])
    assert seen.sum() > 0.9 * on.sum()
    inside = (want[:, 0] > -1) & (want[:, 0] < W) & (want[:, 1] > -1) & (want[:, 1] < H)
    assert np.array_equal(seen, inside) or np.abs(want[seen != inside]).size < 8
    err = np.abs(got[seen] - want[seen]).max()
    flow = np.abs(got[seen] - np.argwhere(on)[seen][:, ::-1]).max(axis=1)
    print(f"max |prev_xy - truth| = {err:.2e} px; image motion of the bodies' pixels: median {np.median(flow):.1f} px, max {flow.max():.1f} px")
    assert err <= 2e-3
    assert np.median(flow) >= 2.0, "the sequence does not move the bodies by several pixels"
    # the static projection of the same pixels is off by that motion: what d_prev_xy was before this stage
    sx, sy, _ = project(gb["position"], prev["cam"], W, H)
    static = np.stack([sx, sy], -1)[on].astype(np.float64)
    assert np.median(np.abs(static[seen] - want[seen]).max(axis=1)) >= 2.0
    assert np.array_equal(_bits(res["prev_position"]), _bits(np.where((gb["range"] <= 3e38)[..., None], X2, F(0))))


def _run_chain(chain, with_bodies):
    """The model chain Q0 -> Q1 -> Q2: the last frame's result and the last frame's motion arguments."""
    first, num = ranges(chain[0]["hs"])
    prev = prev_cam = prev_poses = None
    for k, fr in enumerate(chain):
        if with_bodies:
            mo = (first, num, fr["poses"] if prev_poses is None else prev_poses, fr["poses"], fr["gb"]["prim_id"])
            res = model.denoise_temporal_bodies(fr["S"], fr["S2"], SPP, _guides(fr), mo, prev_cam, prev, **DN)
        else:
            res = denoise_temporal(fr["S"], fr["S2"], SPP, _guides(fr), prev_cam, prev, **DN)
        prev, prev_cam, prev_poses = res["next"], fr["cam"], fr["poses"]
    return res


def test_what_the_stage_buys_on_the_model(dsrt, chain):
    """Of the last frame's filterable pixels on moved bodies whose X' projects at least one pixel inside the previous image: with the bodies stage at least half
    find history, with the static stage on the same inputs fewer than a tenth.  Measured: 436 pixels, 0.528 with the bodies stage, 0.000 with the static stage."""
    with_b, static = _run_chain(chain, True), _run_chain(chain, False)
    cur = chain[2]
    first, num = ranges(cur["hs"])
    body = model.body_of(cur["gb"]["prim_id"], first, num)
    pxy = with_b["prev_xy"]
    with np.errstate(invalid="ignore"):
        inside = (pxy[..., 0] >= 1) & (pxy[..., 0] <= W - 2) & (pxy[..., 1] >= 1) & (pxy[..., 1] <= H - 2)
        pixels = (body >= 1) & (cur["gb"]["range"] <= 3e38) & inside
    n = int(pixels.sum())
    frac_b = float((with_b["weight"][pixels] > SPP).sum()) / n
    frac_s = float((static["weight"][pixels] > SPP).sum()) / n
    print(f"{n} pixels on moved bodies: {frac_b:.3f} find history with the bodies stage, {frac_s:.3f} with the static stage")
    assert n > 100
    assert frac_b >= 0.5
    assert frac_s < 0.1
    # the static pixels (body 0) are the static stage's, bit for bit, where no moved body is involved
    same = body == 0
    assert np.array_equal(_bits(with_b["prev_xy"])[same], _bits(static["prev_xy"])[same])


# ---- 5. the host code under sanitizers, as a program of its own ----
def test_host_form_is_clean_under_asan_and_ubsan(tmp_path):
    """host/body_motion.cpp (with the host sources it links against) in a plain program built with -fsanitize=address,undefined: exact-sized heap arrays, prim_id at
    both ends of int, a range that reaches past INT_MAX (tests/body_motion_sanitize_driver.cpp)."""
    import glob
    srcs = sorted(glob.glob(os.path.join(ROOT, "deep-space-ray-tracer_amd", "host", "*.cpp"))) + [os.path.join(ROOT, "tests", "body_motion_sanitize_driver.cpp")]
    flags = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    procs = [(s, str(tmp_path / (os.path.basename(s) + ".o"))) for s in srcs]
    running = [(s, subprocess.Popen(["g++", *flags, "-c", s, "-o", o], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)) for s, o in procs]
    for s, p in running:
        log, _ = p.communicate()
        assert p.returncode == 0, f"{s}:\n{log}"
    exe = str(tmp_path / "body_motion_sanitize_driver")
    r = subprocess.run(["g++", *flags, *[o for _, o in procs], "-o", exe, "-lz", "-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
