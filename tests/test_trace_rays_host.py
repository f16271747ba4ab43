"""The host side of the ray queries (include/dsrt.h, dsrt_trace_rays) and of the pose helpers that feed them: the binding's structs, the exports,
argument checks that need no device, and dsrt_pose_points_to_model / dsrt_pose_dirs_to_model against the reference's own pose transform.  No GPU involved."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

from conftest import GOLDEN

NEW_EXPORTS = ("dsrt_trace_rays", "dsrt_trace_rays_to_host", "dsrt_pose_points_to_model", "dsrt_pose_dirs_to_model")


def test_ray_structs_match_the_library(dsrt):
    from dsrt_amd import capi
    ptr = C.sizeof(C.c_void_p)
    assert dsrt.lib.dsrt_sizeof(7) == C.sizeof(capi.DsrtRays) == 4 * ptr
    assert dsrt.lib.dsrt_sizeof(8) == C.sizeof(capi.DsrtRayHits) == 9 * ptr
    assert [n for n, _ in capi.DsrtRays._fields_] == ["origins", "dirs", "t_min", "t_max"]
    assert [n for n, _ in capi.DsrtRayHits._fields_] == ["t", "range", "position", "normal", "uv", "albedo", "prim_id", "material_id", "flags"]
    assert list(capi.RAY_HIT_CHANNELS) == [n for n, _ in capi.DsrtRayHits._fields_]
    for n, spec in capi.RAY_HIT_CHANNELS.items():
        assert spec == capi.GBUFFER_CHANNELS[n]                           # per-ray values as the G-buffer table defines them
    assert (capi.TRACE_CLOSEST, capi.TRACE_ANY) == (0, 1)
    assert capi.ABI_VERSION == dsrt.lib.dsrt_abi_version() == 8             # additive: the version stays


def test_new_exports_are_present(dsrt):
    from dsrt_amd import capi
    for name in NEW_EXPORTS:
        assert name in capi.EXPORTS and hasattr(dsrt.lib, name)


def _host_rays(n=4):
    o = np.zeros((n, 3), np.float32)
    d = np.tile(np.array([0, 0, -1], np.float32), (n, 1))
    return o, d


def test_trace_rays_on_a_null_context_is_invalid(dsrt):
    from dsrt_amd import capi
    o, d = _host_rays()
    t = np.zeros(4, np.float32)
    rays = capi.DsrtRays(origins=o.ctypes.data, dirs=d.ctypes.data)
    hits = capi.DsrtRayHits(t=t.ctypes.data)
    assert dsrt.lib.dsrt_trace_rays(None, 4, C.byref(rays), 0, C.byref(hits), None, None) == -1
    assert b"null" in dsrt.lib.dsrt_last_error()
    assert dsrt.lib.dsrt_trace_rays_to_host(None, 4, C.byref(rays), 0, C.byref(hits), None) == -1
    assert b"null" in dsrt.lib.dsrt_last_error()
    for mode in (0, 1):
        assert dsrt.lib.dsrt_trace_rays(None, 0, None, mode, None, None, None) == -1
        assert dsrt.lib.dsrt_trace_rays_to_host(None, 0, None, mode, None, None) == -1


def _poses(dsrt):
    return dsrt.read_pose_file(os.path.join(GOLDEN, "rendezvous_1s_dt0_01s.txt"))


def test_points_to_model_equals_the_references_cam_in_model_for_every_pose(dsrt):
    """dsrt_pose_points_to_model(cam_pos_world) == the cam_in_model the reference's own host code produced (tests/golden/ref_poses_640x360.json), bit for bit."""
    poses = _poses(dsrt)
    ref = json.load(open(os.path.join(GOLDEN, "ref_poses_640x360.json")))
    assert len(poses) == len(ref) == 99
    for p, r in zip(poses, ref):
        assert r["frame"] == ref.index(r)
        cam = np.array(p.cam_pos_world[:], np.float64)
        got = dsrt.pose_to_model(p, cam)
        assert got.dtype == np.float32 and got.shape == (3,)
        assert got.view(np.uint32).tolist() == r["cam_in_model"], r["frame"]
        out = np.empty(3, np.float32)
        assert dsrt.lib.dsrt_pose_points_to_model(C.byref(p), 1, cam.ctypes.data, out.ctypes.data) == 0
        assert out.view(np.uint32).tolist() == r["cam_in_model"]


def _restated(pose, xyz, direction):
    """The yaw rotation of the pose transform, restated in numpy float64: yaw_about_y(v, -yaw), v = p - model_pos_world for points; then float32."""
    rad = -float(pose.model_euler_deg[0]) * 3.1415926535897932385 / 180.0
    c, s = math.cos(rad), math.sin(rad)
    v = xyz if direction else xyz - np.array(pose.model_pos_world[:], np.float64)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    return np.stack([c * x + s * z, y, -s * x + c * z], axis=1).astype(np.float32)


@pytest.mark.parametrize("direction", [False, True])
def test_pose_helpers_equal_a_float64_restatement(dsrt, direction):
    poses = _poses(dsrt)
    rng = np.random.default_rng(1234 + direction)
    for k in (0, 17, 50, 98):
        p = poses[k]
        pts = rng.normal(size=(257, 3)) * np.array([1e3, 50.0, 1e3]) + (0.0 if direction else np.array(p.model_pos_world[:]))
        pts[0] = 0.0
        pts[1] = [-0.0, 1.0, -0.0]
        got = dsrt.pose_to_model(p, pts, direction=direction)
        want = _restated(p, pts, direction)
        assert got.shape == (257, 3) and got.dtype == np.float32
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), k
    # a yaw that is not a multiple of 90 degrees, so that the rotation really mixes x and z
    p = dsrt.DsrtPose()
    p.model_pos_world[:] = [10.0, -3.0, 7.5]
    p.model_euler_deg[:] = [33.25, 0.0, 0.0]
    pts = rng.normal(size=(64, 3)) * 100.0
    assert np.array_equal(dsrt.pose_to_model(p, pts, direction=direction).view(np.uint32), _restated(p, pts, direction).view(np.uint32))


def test_directions_are_rotated_not_translated_or_normalised(dsrt):
    p = dsrt.DsrtPose()
    p.model_pos_world[:] = [1e6, 2e6, 3e6]
    p.model_euler_deg[:] = [90.0, 0.0, 0.0]
    d = dsrt.pose_to_model(p, [2.0, 5.0, 0.0], direction=True)
    assert np.allclose(d, [0.0, 5.0, 2.0], atol=1e-6)                      # yaw_about_y((2, 5, 0), -90): x -> z
    assert abs(float(np.linalg.norm(d)) - math.sqrt(29.0)) < 1e-5


def test_pose_to_model_refuses_bad_shapes(dsrt):
    p = _poses(dsrt)[0]
    for bad in (np.zeros(2), np.zeros((4, 2)), np.zeros((2, 3, 3)), np.zeros(()), np.zeros((0, 4))):
        with pytest.raises(ValueError):
            dsrt.pose_to_model(p, bad)
        with pytest.raises(ValueError):
            dsrt.pose_to_model(p, bad, direction=True)
    assert dsrt.pose_to_model(p, np.zeros((0, 3))).shape == (0, 3)


def test_pose_helpers_refuse_bad_arguments(dsrt):
    lib = dsrt.lib
    p = _poses(dsrt)[0]
    src, dst = np.zeros(3), np.zeros(3, np.float32)
    for fn in (lib.dsrt_pose_points_to_model, lib.dsrt_pose_dirs_to_model):
        assert fn(None, 1, src.ctypes.data, dst.ctypes.data) == -1
        assert fn(C.byref(p), -1, src.ctypes.data, dst.ctypes.data) == -1
        assert fn(C.byref(p), 1, None, dst.ctypes.data) == -1
        assert fn(C.byref(p), 1, src.ctypes.data, None) == -1
        assert fn(C.byref(p), 0, None, None) == 0
