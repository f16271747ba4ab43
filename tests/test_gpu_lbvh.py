"""The GPU-built LBVH (csrc/bvh_lbvh.hip, dsrt_host_scene_build_bvh_gpu) against its bit-exact CPU model (tests/_oracle_lbvh.py).

Every case requires the node array's bytes, tri_indices and stack_need to be the model's: a wrong Morton code, sort, split, box (a stale
one from fit_kernel's hand-off between workgroups included), collapse or numbering fails here even where the tree stays valid and every
image test passes because the oracle walks the same wrong tree.  Plus one end-to-end check that a scene of a single flat quad is hit on
the LBVH tree (its N <= 4 path once built that leaf with zero thickness, which the slab test never enters)."""
import ctypes as C
import os

import numpy as np
import pytest

import _lbvh_scenes as S
from _oracle_lbvh import DepthError, lbvh_model, scene_verts
from conftest import ASSETS
from test_gpu_gbuffer import assert_same, expected_gbuffer
from test_gpu_trace_rays import ALL, expected_hits

pytestmark = pytest.mark.gpu

F = np.float32
CASES = S.synthetic_cases()


def _scene(dsrt, verts):
    return dsrt.HostScene().add_arrays(tris=S.tri_records(verts, dsrt.capi), mats=S.one_material(dsrt.capi))


def assert_model(hs, want, what=""):
    """hs holds an LBVH build: its nodes (bytes), tri_indices and stack need are the model's `want` = (nodes, tri_indices, height)."""
    nodes, idx, height = want
    a = hs.arrays()
    assert np.array_equal(a["idx"], idx), f"{what}: tri_indices differ at {np.flatnonzero(a['idx'] != idx)[:5].tolist()}"
    assert len(a["nodes"]) == len(nodes), (what, len(a["nodes"]), len(nodes))
    got_w, want_w = a["nodes"].view(np.uint32).reshape(-1, 10), nodes.view(np.uint32).reshape(-1, 10)
    bad = np.argwhere(got_w != want_w)
    assert not bad.size, f"{what}: {len(bad)} node words differ, first node {bad[0][0]} word {bad[0][1]}: {a['nodes'][bad[0][0]]} != {nodes[bad[0][0]]}"
    assert a["nodes"].tobytes() == nodes.tobytes()
    assert hs.stack_need == max(height - 1, 0)


@pytest.mark.parametrize("name", sorted(CASES))
def test_synthetic_scenes_equal_the_model(dsrt, gpu_ctx, name):
    verts = CASES[name]
    try:
        want = lbvh_model(verts)
    except DepthError:
        want = None
    hs = _scene(dsrt, verts)
    if want is not None:
        hs.build_bvh("lbvh")
        assert_model(hs, want, name)
        return
    # deeper than the 64-entry stack: the build says so (DSRT_ERR_BVH_DEPTH) and the scene cannot be uploaded
    with pytest.raises(dsrt.DsrtError) as e:
        hs.build_bvh("lbvh")
    assert e.value.code == -5 and hs.stack_need > 64
    view = dsrt.GPUScene()
    assert dsrt.lib.dsrt_host_scene_view(hs._h, C.byref(view)) == 0        # (HostScene.view would rebuild with the median builder)
    with pytest.raises(dsrt.DsrtError) as e:
        gpu_ctx.upload(view)
    assert e.value.code == -5


def test_device_min_keeps_minus_zero_on_the_lower_face(dsrt, gpu_ctx):
    """The sign of zero the device's fminf / fmaxf return for -0.0 against +0.0 (the model orders -0.0 below +0.0), on the single-leaf
    path and through fit_kernel's unions."""
    hs = _scene(dsrt, S.small_signed_zeros())
    hs.build_bvh("lbvh")
    assert hs.arrays()["nodes"][0]["bbox_min"][0].view(np.uint32) == 0x80000000
    verts = S.signed_zeros(300, 1)
    hs = _scene(dsrt, verts)
    hs.build_bvh("lbvh")
    nodes = hs.arrays()["nodes"]
    assert (nodes["bbox_min"].view(np.uint32) == 0x80000000).any()
    assert_model(hs, lbvh_model(verts), "signed zeros")


@pytest.mark.parametrize("world", ["c1_spheres", "lights", "mixed", "quirks", "station_3k", "textured"])
def test_parity_worlds_equal_the_model(dsrt, world):
    cwd = os.getcwd()
    os.chdir(ASSETS)
    try:
        hs = dsrt.HostScene().add_world_file(world + ".world")
    finally:
        os.chdir(cwd)
    hs.build_bvh("lbvh")
    assert_model(hs, lbvh_model(scene_verts(hs.arrays()["tris"])), world)


@pytest.fixture(scope="module")
def stations(dsrt, tmp_path_factory):
    from dsrt_amd import meshgen
    out = {}
    for n in (100000, 1000000):
        obj = tmp_path_factory.mktemp("lbvh") / f"iss_{n}.obj"
        meshgen.generate(obj, n)
        hs = dsrt.HostScene().add_obj(obj)
        hs.build_bvh("lbvh")
        out[n] = (hs, lbvh_model(scene_verts(hs.arrays()["tris"])))
    return out


@pytest.mark.parametrize("n", [100000, 1000000])
def test_station_trees_equal_the_model_on_every_build(dsrt, stations, n):
    """>= 400 (100k) and 4,000 (1M) workgroups per kernel: fit_kernel's hand-off crosses CUs and XCDs.  Every box word is compared, three
    builds each."""
    hs, want = stations[n]
    assert len(want[0]) > n // 4
    for build in range(3):
        if build:
            hs.build_bvh("lbvh")
        assert_model(hs, want, f"{n} triangles, build {build}")


def test_flat_quad_is_hit_on_the_lbvh_tree(dsrt, gpu_ctx, oracle):
    """One axis-aligned quad (2 triangles in the plane z = 0): the N <= 4 path pads its leaf like every other, so the G-buffer, the
    render and trace_rays see it -- equal to the oracle on that tree, and trace_rays equal to its answers on the SAH tree."""
    verts = S.quad(0.0, 1.0, 2)
    hs = _scene(dsrt, verts)
    hs.build_bvh("lbvh")
    assert_model(hs, lbvh_model(verts), "quad")
    W, H, spp, depth = 48, 32, 2, 5
    cam = dsrt.camera_look_at((0.3, -0.4, 4.0), (0.0, 0.0, 0.0), 45.0, W, H, spp, depth)
    sun = (0.2, 0.1, -0.97)                                              # onto the lit (+z) face
    scene = hs.view(cam, sun)
    gpu_ctx.upload(scene)
    g = gpu_ctx.gbuffer_to_host(dsrt.make_desc(W, H, spp, depth))
    assert_same(g, expected_gbuffer(oracle, hs, scene, W, H))
    assert (g["flags"] & 1).sum() > 200                                   # the quad fills much of the frame
    want_rgb, want_f32, _ = oracle.render(scene, W, H)
    rgb, f32, _ = gpu_ctx.render_to_host(dsrt.make_desc(W, H, spp, depth), want_f32=True)
    assert np.array_equal(rgb, want_rgb) and np.array_equal(f32.view(np.uint32), want_f32.view(np.uint32))
    assert want_rgb.max() > 0
    rng = np.random.default_rng(3)
    n = 500
    target = np.concatenate([rng.uniform(-0.99, 0.99, (n, 2)), np.zeros((n, 1))], axis=1)
    O = (target + rng.normal(size=(n, 3)) * np.array([1.0, 1.0, 0.0]) + np.array([0.0, 0.0, 3.0]) * np.where(rng.random((n, 1)) < 0.5, 1, -1)).astype(F)
    D = (target - O).astype(F)
    got = gpu_ctx.trace_rays(O, D)
    assert_same(got, expected_hits(oracle, hs, scene, O, D), keys=ALL)
    assert (got["flags"] & 1).all()
    hs_sah = _scene(dsrt, verts)
    hs_sah.build_bvh("sah")
    gpu_ctx.upload(hs_sah.view(cam, sun))
    assert_same(gpu_ctx.trace_rays(O, D), got, keys=ALL)
