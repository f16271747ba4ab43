"""Movable rigid bodies on the GPU, on the catalogue of tests/_bodies_shapes.py (csrc/bodies_kernel.hip, csrc/api_bodies.hip): launches of several workgroups that
start at an offset, a chain of 15 top nodes, big leaves beyond index 0 and below internal nodes, empty bodies, trees without a chain or without internal records,
-0, flat, mirrored, subnormal and very large coordinates.  The two routes of tests/test_gpu_bodies.py -- upload with bodies then pose on the device, against pose on
the host then plain upload -- compared word for word; then what reads the resident scene, against the CPU oracle on the host-posed scene.  What each entry holds is
proved in tests/test_bodies_shapes_host.py."""
import numpy as np
import pytest

import _bodies_shapes as S
from test_gpu_bodies import ARRAYS, _bounds, _words
from test_gpu_gbuffer import assert_same, expected_gbuffer
from test_gpu_trace_rays import ALL as RAY_ALL
from test_gpu_trace_rays import expected_hits, random_rays, scene_box

pytestmark = pytest.mark.gpu

F = np.float32
W, H, SPP, DEPTH = 48, 32, 8, 8


@pytest.fixture(scope="module")
def ctx_b(dsrt):
    ctx = dsrt.Context(0)
    yield ctx
    ctx.close()


def _upload_rest(dsrt, ctx, name, cam):
    hs = S.build(dsrt, name)
    ctx.upload_bodies(hs, hs.view(cam, S.SUN))
    assert ctx.body_count == len(S.ENTRIES[name])
    return hs


def _assert_same_scene(dsrt, ctx, ctx_b, posed, cam, what):
    """ctx's resident scene against `posed` (a host scene) given a plain upload on ctx_b: the three arrays and the bounds."""
    ctx_b.upload(posed.view(cam, S.SUN))
    assert ctx_b.body_count == 0
    for array, a, b in zip(ARRAYS, _words(ctx), _words(ctx_b)):
        assert a.size == b.size and (a.size > 0 or array == 0), (what, array)
        bad = np.nonzero(a != b)[0]
        assert bad.size == 0, f"{what}, array {array}: {bad.size} of {a.size} words differ, first at {bad[:8].tolist()}"
    assert np.array_equal(_bounds(dsrt, ctx), _bounds(dsrt, ctx_b)), what


def _posed_host(dsrt, name, *pose_dicts):
    hs = S.build(dsrt, name)
    for p in pose_dicts:
        S.apply(hs, p)
    return hs


@pytest.mark.parametrize("name, family", S.CASES)
def test_device_update_equals_host_update_then_upload_word_for_word(dsrt, gpu_ctx, ctx_b, name, family):
    p = S.poses(name, family)
    posed = _posed_host(dsrt, name, p)
    cam = S.camera(dsrt, S.build(dsrt, name), W, H)
    rest = _upload_rest(dsrt, gpu_ctx, name, cam)
    _assert_same_scene(dsrt, gpu_ctx, ctx_b, rest, cam, (name, "at rest"))
    S.apply(gpu_ctx, p)
    _assert_same_scene(dsrt, gpu_ctx, ctx_b, posed, cam, (name, family))


def test_sixteen_all_at_once_then_the_last_then_three_then_none(dsrt, gpu_ctx, ctx_b):
    cam = S.camera(dsrt, S.build(dsrt, "sixteen"), W, H)
    _upload_rest(dsrt, gpu_ctx, "sixteen", cam)
    host = S.build(dsrt, "sixteen")
    p, q, r = (S.poses("sixteen", seed=k) for k in (0, 1, 2))
    calls = [("all 15", 1, np.stack([p[b] for b in range(1, 16)])), ("body 15 alone", 15, q[15][None]), ("bodies 7 to 9", 7, np.stack([r[b] for b in (7, 8, 9)])),
             ("count 0", 4, np.zeros((0, 12), F))]
    for what, first, poses in calls:
        gpu_ctx.set_body_poses(first, poses)
        host.set_body_poses(first, poses)
        _assert_same_scene(dsrt, gpu_ctx, ctx_b, host, cam, what)


def test_wide_second_body_alone_then_the_first_then_both(dsrt, gpu_ctx, ctx_b):
    cam = S.camera(dsrt, S.build(dsrt, "wide"), W, H)
    _upload_rest(dsrt, gpu_ctx, "wide", cam)
    host = S.build(dsrt, "wide")
    p = S.poses("wide")
    for what, first, poses in (("body 2 alone", 2, p[2][None]), ("then body 1 alone", 1, p[1][None])):      # body 2's transform launch starts beyond entry 256
        gpu_ctx.set_body_poses(first, poses)
        host.set_body_poses(first, poses)
        _assert_same_scene(dsrt, gpu_ctx, ctx_b, host, cam, what)
    one_by_one = _words(gpu_ctx), _bounds(dsrt, gpu_ctx)
    _upload_rest(dsrt, gpu_ctx, "wide", cam)
    S.apply(gpu_ctx, p)                                                                       # both in one call: the same end state
    for a, b in zip(one_by_one[0], _words(gpu_ctx)):
        assert np.array_equal(a, b)
    assert np.array_equal(one_by_one[1], _bounds(dsrt, gpu_ctx))


def test_wide_on_a_side_stream_with_times(dsrt, gpu_ctx, ctx_b):
    """Plumbing only: the update given a stream of its own and `ms` leaves the words of the NULL-stream call, and the times it reports are times."""
    import torch
    cam = S.camera(dsrt, S.build(dsrt, "wide"), W, H)
    p = S.runs(S.poses("wide"))
    assert len(p) == 1
    _upload_rest(dsrt, gpu_ctx, "wide", cam)
    assert gpu_ctx.set_body_poses(*p[0]) is None
    want = _words(gpu_ctx), _bounds(dsrt, gpu_ctx)
    _upload_rest(dsrt, gpu_ctx, "wide", cam)
    side = torch.cuda.Stream(device="cuda:0")
    ms, transform, refit, chain = gpu_ctx.set_body_poses(*p[0], stream=side.cuda_stream, want_ms=True)
    side.synchronize()
    for a, b in zip(want[0], _words(gpu_ctx)):
        assert np.array_equal(a, b)
    assert np.array_equal(want[1], _bounds(dsrt, gpu_ctx))
    assert all(np.isfinite(t) and t >= 0 for t in (ms, transform, refit, chain))
    assert transform + refit + chain <= ms * (1 + 1e-3) + 1e-3                                # (event times are rounded to the device clock)


def test_posing_an_empty_body_changes_nothing(dsrt, gpu_ctx, oracle):
    cam = S.camera(dsrt, S.build(dsrt, "holes"), W, H)
    hs = _upload_rest(dsrt, gpu_ctx, "holes", cam)
    before, box = _words(gpu_ctx), _bounds(dsrt, gpu_ctx)
    for b in (1, 3, 5):
        assert hs.body_range(b)[1] == 0
        gpu_ctx.set_body_poses(b, S.poses("holes")[b][None])                                  # no triangle to transform: no transform launch; refit and chain still run
        for a, c in zip(before, _words(gpu_ctx)):
            assert np.array_equal(a, c)
        assert np.array_equal(box, _bounds(dsrt, gpu_ctx))
    got = gpu_ctx.gbuffer_to_host(dsrt.make_desc(W, H, SPP, DEPTH))
    want = expected_gbuffer(oracle, hs, hs.view(cam, S.SUN), W, H)
    assert (want["prim_id"] >= 0).any()
    assert_same(got, want)


def _moved_range(hs, p):
    """(lo, hi): the triangles of the bodies that p poses, which follow the static part."""
    live = [hs.body_range(b) for b in p if hs.body_range(b)[1] > 0]
    return min(f for f, _ in live), max(f + n for f, n in live)


CONSUMERS = [("sixteen", "rigid"), ("big_leaves", "rigid"), ("one_live", "rigid"), ("one_leaf", "rigid"), ("sixteen", "collapse")]


@pytest.mark.parametrize("name, family", CONSUMERS)
def test_gbuffer_and_ray_queries_on_the_posed_scene(dsrt, gpu_ctx, oracle, name, family):
    p = S.poses(name, family)
    posed = _posed_host(dsrt, name, p)
    cam = S.camera(dsrt, posed, W, H)
    _upload_rest(dsrt, gpu_ctx, name, cam)
    S.apply(gpu_ctx, p)
    scene = posed.view(cam, S.SUN)
    lo, hi = _moved_range(posed, p)
    got = gpu_ctx.gbuffer_to_host(dsrt.make_desc(W, H, SPP, DEPTH))
    want = expected_gbuffer(oracle, posed, scene, W, H)
    assert ((want["prim_id"] >= lo) & (want["prim_id"] < hi)).any(), "no pixel sees a moved body"
    assert_same(got, want)
    O, D = random_rays(*scene_box(posed), 1000, 17)
    hits = gpu_ctx.trace_rays(O, D)
    want = expected_hits(oracle, posed, scene, O, D)
    assert want["flags"].any() and not want["flags"].all() and ((want["prim_id"] >= lo) & (want["prim_id"] < hi)).any()
    assert_same(hits, want, keys=RAY_ALL)
    assert np.array_equal(gpu_ctx.trace_rays(O, D, any_hit=True)["flags"], want["flags"] & 1)


@pytest.mark.parametrize("name", ["sixteen", "one_leaf"])
def test_render_of_the_posed_scene_is_the_oracles(dsrt, gpu_ctx, oracle, name):
    p = S.poses(name)
    posed = _posed_host(dsrt, name, p)
    cam = S.camera(dsrt, posed, W, H)
    _upload_rest(dsrt, gpu_ctx, name, cam)
    S.apply(gpu_ctx, p)
    scene = posed.view(cam, S.SUN)
    rgb, f32, st = gpu_ctx.render_to_host(dsrt.make_desc(W, H, SPP, DEPTH, checked=1), want_f32=True)
    want_rgb, want_f32, _ = oracle.render(scene, W, H)
    assert st.device_flags == 0
    lo, hi = _moved_range(posed, p)
    prim = expected_gbuffer(oracle, posed, scene, W, H)["prim_id"]
    assert ((prim >= lo) & (prim < hi)).any() and (want_rgb.max(axis=2) > 0).any()
    assert np.array_equal(rgb, want_rgb) and np.array_equal(f32.view(np.uint32), want_f32.view(np.uint32))
