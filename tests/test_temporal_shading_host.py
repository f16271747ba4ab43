"""Temporal accumulation that follows shading on the CPU (include/dsrt.h, TEMPORAL ACCUMULATION THAT FOLLOWS SHADING): the exports, everything the entry points
refuse without a device, the CLI's usage errors, the properties of the numpy model of tests/_shading_model.py on synthetic frames -- its reductions to the two
stages below it, the state test tap by tap, the status byte -- and what the rule buys on the three-frame chain of the bodies scene against a 256-spp image of the
last frame, all on the oracle's G-buffers and sums, no GPU.  Every float comparison is on uint32 views."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _bodies_model as B
import _motion_model as motion_model
import _shading_model as model
from _denoise_model import DEFAULTS as DN, F, start
from _sample_sets import SetOracle
from _temporal_model import denoise_temporal, random_history, wall_frame
from conftest import ROOT
from test_temporal_bodies_host import DEPTH, H, SEED, SPP, W, _guides, chain, lookfrom, ranges  # noqa: F401  (chain: the module's fixture, computed once here too)

NEW_EXPORTS = ("dsrt_denoise_temporal_shaded", "dsrt_denoise_temporal_shaded_to_host", "dsrt_ctx_set_temporal_shading", "dsrt_ctx_temporal_shading")


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _same(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = g != w
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at {np.argwhere(bad)[0].tolist()}"


# ---- 1. ABI ----
def test_struct_size_and_exports(dsrt):
    capi = dsrt.capi
    assert dsrt.lib.dsrt_sizeof(19) == C.sizeof(capi.DsrtTemporalShading) == 2 * C.sizeof(C.c_void_p)
    assert [f for f, _ in capi.DsrtTemporalShading._fields_] == ["flags", "edge_guard"]
    assert capi.ABI_VERSION == dsrt.lib.dsrt_abi_version() == 8                       # additive: the version stays
    for name in NEW_EXPORTS:
        assert name in capi.EXPORTS and hasattr(dsrt.lib, name)
    for m in ("denoise_temporal_shaded", "denoise_temporal_shaded_to_host", "set_temporal_shading", "temporal_shading"):
        assert hasattr(dsrt.Context, m)
    sh = dsrt.temporal_shading(None, 1)
    assert isinstance(sh, capi.DsrtTemporalShading) and sh.edge_guard == 1 and not sh.flags
    assert dsrt.lib.dsrt_ctx_temporal_shading(None) == 0 and dsrt.lib.dsrt_ctx_set_temporal_shading(None, 1) == -1


# ---- 2. refusals ----
def test_refusals_that_need_no_device(dsrt):
    """Every argument check of dsrt_denoise_temporal_shaded comes before the context or any buffer is looked at: a stand-in for the context and host arrays do."""
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
    flags, status = np.full(px + 8, 0x33, np.uint8), np.full(px + 8, 0x5A, np.uint8)
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
             bodies=3, first=first, num=num, pp=pp, pc=pc, prim=prim, motion=True, flags=flags, flags_off=0, guard=1, null_shading=False, status=status, status_off=0, fn="dev"):
        a = capi.DsrtAccum(ptr(S), ptr(sq))
        g = capi.DsrtDenoiseGuides(*[ptr(x) for x in guides])
        m = capi.DsrtBodyMotion(bodies, ptr(first), ptr(num), ptr(pp), ptr(pc), ptr(prim))
        sh = capi.DsrtTemporalShading(ptr(flags, flags_off), guard)
        tp = T() if tp == "default" else tp
        dn = dsrt.denoise_defaults() if dn == "default" else dn
        args = [ctx, ref(desc), ref(a), done, None, ref(g), ref(m) if motion else None, None if null_shading else ref(sh), ref(cam), ptr(prev), ptr(nxt), ref(tp), ref(dn)] + \
               [ptr(o) for o in outs] + [ptr(pxy), ptr(wgt), ptr(ppos), ptr(status, status_off)]
        return lib.dsrt_denoise_temporal_shaded(*args, None) if fn == "dev" else lib.dsrt_denoise_temporal_shaded_to_host(*args)

    cases = {}
    for fn in ("dev", "host"):
        c = lambda **kw: call(fn=fn, **kw)                                          # noqa: E731
        cases.update({(fn, k): v for k, v in {
            # what dsrt_denoise_temporal_bodies refuses, one of each class
            "NULL sum_sq": c(sq=None), "NULL guide": c(guides=(N, X, None, R)), "rng_mode 0": c(desc=dsrt.make_desc(w, h, 4, rng_mode=0)), "samples_done 1": c(done=1),
            "iterations 7": c(dn=dsrt.denoise_defaults(iterations=7)), "no output": c(outs=(None,) * 4), "output over an input": c(outs=(rgb, None, N, var)),
            "camera without history": c(prev=None), "history without camera": c(cam=None), "NULL next": c(nxt=None), "NULL DsrtTemporal": c(tp=None),
            "alpha_min NaN": c(tp=T(alpha_min=float("nan"))), "plane_tol 0": c(tp=T(plane_tol=0.0)), "next is prev": c(nxt=hp), "prev_xy over weight": c(wgt=pxy),
            "NULL first_tri": c(first=None), "NULL prim_id": c(prim=None), "bodies 0": c(bodies=0), "bodies 17": c(bodies=17), "negative num_tris": c(num=changed(num, 2, -3)),
            "ranges overlap": c(first=changed(first, 2, 19)), "NaN pose": c(pc=changed(pc, 13, np.nan)), "weight over prim_id": c(wgt=prim.view(F)),
            "prev_position over next": c(ppos=hn), "first frame: NaN pose": c(cam=None, prev=None, pp=changed(pp, 20, np.nan)),
            # the shading's
            "NULL shading": c(null_shading=True), "NULL flags": c(flags=None), "edge_guard 2": c(guard=2), "edge_guard -1": c(guard=-1),
            "NULL shading, no motion": c(null_shading=True, motion=False, ppos=None), "first frame: NULL flags": c(cam=None, prev=None, flags=None),
            "prev_position without a motion": c(motion=False), "flags over linear": c(flags=lin.view(np.uint8)), "flags over rgb8": c(flags=rgb),
            "flags over next": c(flags=hn.view(np.uint8)), "flags over prev_xy": c(flags=pxy.view(np.uint8)), "flags over weight": c(flags=wgt.view(np.uint8)),
            "flags over prev_position": c(flags=ppos.view(np.uint8)), "flags over status": c(status=flags), "flags and status share a byte": c(status=flags, status_off=px - 1),
            "status over an input": c(status=N.view(np.uint8)), "status over the sums": c(status=S.view(np.uint8)), "status over prim_id": c(status=prim.view(np.uint8)),
            "status over prev": c(status=hp.view(np.uint8)), "status over next": c(status=hn.view(np.uint8)), "status over linear": c(status=lin.view(np.uint8)),
            "status over rgb8": c(status=rgb, status_off=px * 3 - 1), "status over weight": c(status=wgt.view(np.uint8)),
            "status over prev_position": c(status=ppos.view(np.uint8)),
        }.items()})
    assert {k: v for k, v in cases.items() if v != -1} == {}
    assert lib.dsrt_last_error()
    # a good call gets as far as a later refusal: with a motion, without one, flags at an odd address, no status
    for kw in (dict(), dict(motion=False, ppos=None), dict(flags_off=3), dict(status=None), dict(guard=0)):
        assert call(nxt=hn[1:], **kw) == -1 and b"16-byte aligned" in lib.dsrt_last_error(), kw
    assert (rgb == 0x5A).all() and (prim == -1).all() and (flags == 0x33).all() and (status == 0x5A).all()
    assert all((a == -7.5).all() for a in (lin, var, hp, hn, pxy, wgt, ppos, N, X, A, R))
    assert lib.dsrt_ctx_set_temporal_shading(None, 0) == -1 and b"null context" in lib.dsrt_last_error()


@pytest.mark.parametrize("flags, says", [
    (["--rng-mode", "1", "--denoise", "--follow-shading"], "--follow-shading needs --denoise and --temporal"),
    (["--rng-mode", "1", "--temporal", "--follow-shading"], "--denoise"),
    (["--rng-mode", "1", "--follow-shading", "--follow-bodies", "--body", "x.obj"], "--follow-shading needs --denoise and --temporal"),
])
def test_cli_usage_errors(flags, says, tmp_path):
    exe = os.path.join(ROOT, "deep-space-ray-tracer_amd", "dsrt_render")
    r = subprocess.run([exe, "--obj", "none.obj", "--output_dir", str(tmp_path)] + flags, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and says in r.stderr, r.stderr


def test_cli_usage_names_the_flag():
    exe = os.path.join(ROOT, "deep-space-ray-tracer_amd", "dsrt_render")
    r = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
    assert "--follow-shading" in r.stdout + r.stderr


# ---- 3. the model on synthetic frames ----
EDGES = {k: model.EDGES[k] for k in ((33, 17), (37, 29))}


def _frame(dsrt, Wd, Hd, special=0.2, miss=0.15):
    """The wall of tests/_temporal_model.py seen from two nearby cameras, a history of it, a prim_id image over four body ranges and poses that move bodies 1 and 3
    in the wall's plane -- the synthetic frame of tests/test_gpu_temporal_bodies.py."""
    rng = np.random.default_rng(1000 * Wd + Hd)
    look = lambda p: dsrt.camera_look_at(p, (0, 0, 0), 40.0, Wd, Hd, 8, 5)            # noqa: E731
    cam1, cam0 = look((0.0, 0.0, 10.2)), look((0.3, -0.2, 10.0))
    S, S2, n, g = wall_frame(rng, cam1, Wd, Hd, miss=miss)
    prev, kind = random_history(rng, wall_frame(rng, cam0, Wd, Hd)[3], special=special)
    first, num = np.array([0, 40, 100, 131], np.int32), np.array([40, 50, 31, 19], np.int32)
    prim = rng.integers(-4, 156, size=(Hd, Wd)).astype(np.int32)
    z = (0.0, 0.0, 1.0)
    in_plane = lambda: B._pose(B._rot(z, rng.uniform(-0.08, 0.08)), (rng.uniform(-0.4, 0.4), rng.uniform(-0.4, 0.4), 0.0))     # noqa: E731
    pp, pc = np.zeros((4, 12), F), np.zeros((4, 12), F)
    for b in (1, 2, 3):
        pp[b], pc[b] = in_plane(), in_plane()
    pc[2] = pp[2]
    return dict(rng=rng, S=S, S2=S2, n=n, g=g, cam0=cam0, prev=prev, kind=kind, mo=(first, num, pp, pc, prim))


@pytest.mark.parametrize("Wd, Hd", sorted(EDGES))
def test_uniform_flags_and_an_old_history_are_the_stages_below(dsrt, Wd, Hd):
    s = _frame(dsrt, Wd, Hd)
    assert not _bits(s["prev"][..., 15]).any()
    with np.errstate(invalid="ignore"):
        hit = s["g"]["range"] <= 3e38
    kw = {**DN, "iterations": 2}
    for sun in (0, 8):
        flags = (hit * 1 | sun).astype(np.uint8)
        for guard in (0, 1):
            want = motion_model.denoise_temporal_bodies(s["S"], s["S2"], 8, s["g"], s["mo"], s["cam0"], s["prev"], **kw)
            got = model.denoise_temporal_shaded(s["S"], s["S2"], 8, s["g"], flags, s["mo"], guard, s["cam0"], s["prev"], **kw)
            assert want["found"].sum() > Wd * Hd // 16
            for k in ("linear", "var", "prev_xy", "weight", "prev_position"):
                _same(got[k], want[k], ("bodies", sun, guard, k))
            _same(got["next"][..., :15], want["next"][..., :15], ("bodies", sun, guard, "next"))
            _same(got["next"][..., 15], np.where(hit, F(2 if sun else 1), F(0)), ("bodies", sun, guard, "word 15"))
            assert np.array_equal(got["found"], want["found"]) and not (got["status"] & 24).any()
            assert np.array_equal((got["status"] & 4) != 0, want["found"]), "status bit 2 is the present stage's decision"
            static = denoise_temporal(s["S"], s["S2"], 8, s["g"], s["cam0"], s["prev"], **kw)
            got = model.denoise_temporal_shaded(s["S"], s["S2"], 8, s["g"], flags, None, guard, s["cam0"], s["prev"], **kw)
            for k in ("linear", "var", "prev_xy", "weight"):
                _same(got[k], static[k], ("static", sun, guard, k))
            _same(got["next"][..., :15], static["next"][..., :15], ("static", sun, guard, "next"))
            assert got["prev_position"] is None and np.array_equal(got["found"], static["found"])
    first = model.denoise_temporal_shaded(s["S"], s["S2"], 8, s["g"], flags, s["mo"], 1, None, None, **kw)
    assert not first["status"].any() and not first["found"].any() and (_bits(first["next"][..., 15]) != 0).any()


@pytest.mark.parametrize("Wd, Hd", sorted(EDGES))
def test_stray_states_obey_the_mismatch_rule_tap_by_tap(dsrt, Wd, Hd):
    """No record is off the plane here, so the occluder guard never fires, and a record the state test skips is then worth exactly a record with m = 0 to the stage
    below: the shaded stage on a history of states drawn from {0, 1, 2, -0, NaN, 3} equals the bodies stage on the history with those records' weights zeroed."""
    s = _frame(dsrt, Wd, Hd, special=0.0)
    rng = s["rng"]
    states = np.array([0x00000000, 0x3F800000, 0x40000000, 0x80000000, 0x7FC00000, 0x40400000], np.uint32).view(F)
    prev = s["prev"].copy()
    prev[..., 15] = states[rng.integers(0, 6, prev.shape[:2])]
    with np.errstate(invalid="ignore"):
        hit = s["g"]["range"] <= 3e38
    kw = {**DN, "iterations": 0}
    for sun, matches in ((8, (0, 2, 3)), (0, (0, 1, 3))):                            # the indices of `states` that match a lit / a shadowed pixel: 0, -0 and its own
        flags = (hit * 1 | sun).astype(np.uint8)
        ok = np.isin(_bits(prev[..., 15]), _bits(states[list(matches)]))
        assert 0.3 < ok.mean() < 0.7
        zeroed = prev.copy()
        zeroed[..., 3] = np.where(ok, prev[..., 3], F(0))
        zeroed[..., 15] = 0
        want = motion_model.denoise_temporal_bodies(s["S"], s["S2"], 8, s["g"], s["mo"], s["cam0"], zeroed, **kw)
        got = model.denoise_temporal_shaded(s["S"], s["S2"], 8, s["g"], flags, s["mo"], 0, s["cam0"], prev, **kw)
        assert not model.INFO["guarded"].any()
        for k in ("linear", "var", "weight", "prev_xy"):
            _same(got[k], want[k], (sun, k))
        assert np.array_equal(got["found"], want["found"])
        geometry = motion_model.denoise_temporal_bodies(s["S"], s["S2"], 8, s["g"], s["mo"], s["cam0"], prev, **kw)["found"]
        assert np.array_equal((got["status"] & 4) != 0, geometry), "status bit 2 is the present stage's decision, whatever the states"
        assert geometry.sum() > Wd * Hd // 2 and 0 < got["found"].sum() < geometry.sum() // 2
        # edge_prev: a usable record of another state anywhere in the 4 x 4 block -- here next to every pixel that taps
        assert ((got["status"] & 8) != 0)[model.INFO["use"]].mean() > 0.95
        # edge_guard 0 never consults bits 3 and 4, edge_guard 1 does
        guarded = model.denoise_temporal_shaded(s["S"], s["S2"], 8, s["g"], flags, s["mo"], 1, s["cam0"], prev, **kw)
        assert np.array_equal(guarded["status"] & ~np.uint8(2), got["status"] & ~np.uint8(2))
        assert np.array_equal(guarded["found"], got["found"] & ((got["status"] & 24) == 0))
        assert (got["found"] & ((got["status"] & 24) != 0)).sum() > Wd * Hd // 16


@pytest.mark.parametrize("Wd, Hd", sorted(EDGES))
def test_status_bits_and_the_edge_guards(dsrt, Wd, Hd):
    s = _frame(dsrt, Wd, Hd, special=0.05, miss=0.1)
    rng = s["rng"]
    flags = model.shadow_flags(rng, s["g"]["range"], EDGES[Wd, Hd])
    prev = model.with_states(rng, s["prev"], model.shadow_flags(rng, s["g"]["range"], EDGES[Wd, Hd], shift=model.EDGE_SHIFT), stray=0.03)
    kw = {**DN, "iterations": 1}
    off = model.denoise_temporal_shaded(s["S"], s["S2"], 8, s["g"], flags, s["mo"], 0, s["cam0"], prev, **kw)
    on = model.denoise_temporal_shaded(s["S"], s["S2"], 8, s["g"], flags, s["mo"], 1, s["cam0"], prev, **kw)
    present = motion_model.denoise_temporal_bodies(s["S"], s["S2"], 8, s["g"], s["mo"], s["cam0"], prev, **kw)
    bit = lambda r, b: (r["status"] & b) != 0                                        # noqa: E731
    assert np.array_equal(bit(on, 4), present["found"]) and np.array_equal(bit(off, 4), present["found"])
    assert np.array_equal(bit(on, 1), ~np.isnan(on["prev_xy"][..., 0])) and np.array_equal(on["status"] & 29, off["status"] & 29)
    assert np.array_equal(bit(on, 2), on["found"]) and np.array_equal(bit(off, 2), off["found"])
    assert np.array_equal(on["found"], off["found"] & ~bit(off, 24)), "edge_guard 1 voids exactly the pixels with an edge bit"
    assert not (bit(off, 2) & ~bit(off, 4)).any(), "the state test only ever removes history"
    use = model.INFO["use"]
    assert not (on["status"][~use] & 30).any() and np.array_equal(bit(on, 16), use & model.edge_cur(flags))
    # without history: the frame's own values, bit for bit; with it: the weight says so
    c, v = start(s["S"], s["S2"], 8)
    lost = ~on["found"]
    _same(on["blended"][0][lost], c[lost], "c without history"); _same(on["blended"][1][lost], v[lost], "v without history")
    assert (on["weight"][on["found"]] > 8).all() and (on["weight"][lost] <= 8).all()
    classes = model.status_classes(on, off, present["found"])
    print({k: int(m.sum()) for k, m in classes.items()}, "of", Wd * Hd)
    assert all(m.sum() >= (1 if k.startswith("only") else Wd * Hd // 16) for k, m in classes.items())     # (each guard is the sole cause somewhere)
    _same(on["next"][..., 15], model.sun_state(flags, s["g"]["range"]), "word 15")
    assert not _bits(on["next"][..., 7]).any() and not _bits(on["next"][..., 11]).any()


# ---- 4. what it buys: the chain Q0 -> Q1 -> Q2 of the bodies scene against 256 samples of Q2 ----
def _run(chain, shaded, guard=1):
    first, num = ranges(chain[0]["hs"])
    prev = prev_cam = prev_poses = None
    for fr in chain:
        mo = (first, num, fr["poses"] if prev_poses is None else prev_poses, fr["poses"], fr["gb"]["prim_id"])
        if shaded:
            res = model.denoise_temporal_shaded(fr["S"], fr["S2"], SPP, _guides(fr), fr["gb"]["flags"], mo, guard, prev_cam, prev, **{**DN, "iterations": 0})
        else:
            res = motion_model.denoise_temporal_bodies(fr["S"], fr["S2"], SPP, _guides(fr), mo, prev_cam, prev, **{**DN, "iterations": 0})
        prev, prev_cam, prev_poses = res["next"], fr["cam"], fr["poses"]
    return res


def test_what_the_rule_buys_on_the_model(dsrt, chain):
    """MSE of the blended mean, before the a-trous iterations, against frame Q2 at 256 spp (seed SEED + 777), over the pixels where the present bodies stage finds
    history -- those on moved bodies and the static hits.  Measured (moved / static): raw 1.09e-3 / 1.05e-3; present stage 6.13e-2 / 4.85e-2 with 230 / 703
    pixels; tap test only 1.03e-3 / 3.50e-3, keeping 180 / 607; the full rule 1.03e-3 / 1.10e-3, keeping 119 / 408."""
    cur = chain[2]
    hs = B.build_scene(dsrt)
    hs.set_body_poses(1, cur["poses"][1:])
    scene = hs.view(dsrt.camera_look_at(lookfrom(2), B.LOOKAT, B.VFOV, W, H, 256, DEPTH), B.SUN)
    scene.seed = SEED + 777
    truth = start(*SetOracle().sums(scene, W, H, 0, 256), 256)[0].astype(np.float64)
    present, taps, full = _run(chain, False), _run(chain, True, 0), _run(chain, True, 1)
    first, num = ranges(cur["hs"])
    body = motion_model.body_of(cur["gb"]["prim_id"], first, num)
    raw = start(cur["S"], cur["S2"], SPP)[0]
    mse = lambda img, px: float(((img[px].astype(np.float64) - truth[px]) ** 2).mean())   # noqa: E731
    assert np.array_equal((full["status"] & 4) != 0, present["found"])
    for name, px, n_want in (("moved", present["found"] & (body >= 1), 230), ("static", present["found"] & (body == 0), 703)):
        n = int(px.sum())
        e_raw, e_present, e_taps, e_full = mse(raw, px), mse(present["blended"][0], px), mse(taps["blended"][0], px), mse(full["blended"][0], px)
        keep_taps, keep_full = int(taps["found"][px].sum()), int(full["found"][px].sum())
        print(f"{name}: {n} pixels; MSE raw {e_raw:.3e}, present {e_present:.3e}, tap test {e_taps:.3e} (keeps {keep_taps}), full rule {e_full:.3e} (keeps {keep_full}: "
              f"{keep_full / n:.2f}); present / full = {e_present / e_full:.1f}, full / raw = {e_full / e_raw:.2f}")
        assert n == n_want
        assert e_full <= e_present / 10
        assert e_full <= 1.25 * e_raw
        assert keep_full >= 0.4 * n
