"""rng_mode 1 (a Philox4x32-10 sub-sequence per (pixel, sample), integer sums) against the CPU oracle, bit for bit.

Mode 1 does not depend on the order of work, and include/dsrt.h (DsrtRenderDesc.rng_mode) writes it out completely; oracle/dsrt_oracle.c
restates that on the CPU (dsrt_oracle_render_rect, pinned against rocRAND's host engine in tests/test_oracle_rng_mode1.py).  So every launch
path of mode 1 is held to the oracle's bytes here -- rgb8 and the float32 image as bit patterns -- in math_mode 0, as the mode-0 suite
(tests/test_gpu_parity.py) holds mode 0: the parity scenes with work counters, sample counts around the slicing and the 32-bit item sums, a
sub-sequence number above 2^32, tile culling, shards, the 8-rank layout, batches, the frame pipeline, the certified tree, the SAH and GPU-built
trees, the scheduling switches and the widest image the pixel packing allows.  math_mode 1 has no CPU counterpart: its distance from the
oracle is bounded.
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_world
from test_oracle import CASES, SUN
from _oracle_mode1 import RectOracle

pytestmark = pytest.mark.gpu

SEED = 0xDEADBEEF00001337            # a key whose high word is nonzero: set in the scene (oracle) and the desc (kernel) alike
COUNTERS = ("samples", "rays", "primary_hits", "box_fetches", "nodes_entered", "internal_entered", "tri_tests", "hit_updates", "sphere_tests",
            "shaded_hits", "tex_fetches", "max_stack")


@pytest.fixture(scope="module")
def rect(dsrt):
    return RectOracle()


def _same(got_rgb, got_f32, want_rgb, want_f32, what):
    assert np.array_equal(got_rgb, want_rgb), f"{what}: {(got_rgb != want_rgb).any(axis=-1).sum()} pixels differ"
    if got_f32 is not None:
        assert np.array_equal(got_f32.view(np.uint32), want_f32.view(np.uint32)), f"{what}: float image differs"


def _case(dsrt, name, spp=None, seed=SEED):
    world, cam_args, spp0 = CASES[name]
    spp = spp0 if spp is None else spp
    hs = load_world(dsrt, world)
    W, H, depth = cam_args[3], cam_args[4], cam_args[5]
    cam = dsrt.camera_look_at(cam_args[0], cam_args[1], cam_args[2], W, H, spp, depth)
    scene = hs.view(cam, SUN)
    scene.seed = seed
    return hs, scene, W, H, spp, depth


_WANT = {}


def _case_want(dsrt, rect, name):
    """_case with the oracle's mode-1 image of it (rendered once per module)."""
    hs, scene, W, H, spp, depth = _case(dsrt, name)
    if name not in _WANT:
        _WANT[name] = rect.render(scene, W, H)
    return (hs, scene, W, H, spp, depth) + _WANT[name]


def _desc(dsrt, W, H, spp, depth, seed=SEED, **kw):
    return dsrt.make_desc(W, H, spp, depth, seed=seed, rng_mode=1, **kw)


@pytest.mark.parametrize("name", sorted(CASES))
def test_parity_scenes_match_the_oracle_with_counters(dsrt, gpu_ctx, rect, name):
    hs, scene, W, H, spp, depth, want, want32, cnt = _case_want(dsrt, rect, name)
    assert want.max() > 0
    gpu_ctx.upload(scene)
    # counting build without the any-hit early-out: the work counters are the oracle's exactly
    rgb, f32, st = gpu_ctx.render_to_host(_desc(dsrt, W, H, spp, depth, collect_counters=2), want_f32=True)
    _same(rgb, f32, want, want32, name)
    for key in COUNTERS:
        assert getattr(st, key) == cnt[key], (key, getattr(st, key), cnt[key])
    # production build, and the bounds-checked one
    for kw in ({}, {"checked": 1}):
        rgb, f32, _ = gpu_ctx.render_to_host(_desc(dsrt, W, H, spp, depth, **kw), want_f32=True)
        _same(rgb, f32, want, want32, (name, kw))


def test_sample_counts_around_the_slicing(dsrt, gpu_ctx, rect):
    """spp not a multiple of the 8 slices, a single sample, one more than a power of two, and more than the 4095 samples an item may hold."""
    hs = load_world(dsrt, "lights")
    uploaded = False
    for W, H, spp in ((40, 24, 1), (40, 24, 7), (40, 24, 9), (40, 24, 13), (40, 24, 257), (12, 8, 4100)):
        cam = dsrt.camera_look_at((0.0, 3.0, 9.0), (0.0, 2.0, 0.0), 45.0, W, H, spp, 12)
        scene = hs.view(cam, SUN)
        scene.seed = SEED
        if not uploaded:
            gpu_ctx.upload(scene)
            uploaded = True
        else:
            gpu_ctx.set_camera_sun(cam, SUN)
        want, want32, cnt = rect.render(scene, W, H)
        rgb, f32, st = gpu_ctx.render_to_host(_desc(dsrt, W, H, spp, 12, collect_counters=1), want_f32=True)
        assert st.samples == W * H * spp == cnt["samples"], spp
        _same(rgb, f32, want, want32, spp)
        rgb, f32, _ = gpu_ctx.render_to_host(_desc(dsrt, W, H, spp, 12, tune=(0, 0, 0, 16)), want_f32=True)
        _same(rgb, f32, want, want32, (spp, "no stealing"))


def _light_scene(dsrt):
    """The camera inside an emissive sphere brighter than 1 in every channel: every sample clamps to exactly 1.0 (2^20 units)."""
    capi = dsrt.capi
    sph = np.zeros(1, capi.SPHERE_DTYPE)
    sph["radius"] = 50.0
    mats = np.zeros(1, capi.MAT_DTYPE)
    mats["type"] = 3
    mats["emissive"] = (4.0, 2.0, 7.0)
    mats["albedo_tex"] = -1
    hs = dsrt.HostScene().add_arrays(spheres=sph, mats=mats)
    hs.build_bvh()
    return hs


def test_item_sums_stay_below_two_to_the_32(dsrt, gpu_ctx, rect):
    """An item's sums are 32-bit in units of 2^-20: 4095 samples of 1.0 fit, 4096 do not.  With one slice per pixel (experiment bits 8-19)
    only the host's 4095 clamp keeps an item below that; spp 5000 cuts a pixel into two items in any case."""
    hs = _light_scene(dsrt)
    W, H = 16, 8
    try:
        for xp in (0, 1 << 8, (1 << 8) | (1 << 31)):
            dsrt.set_experiment(xp)
            for spp in (4095, 4096, 5000):
                cam = dsrt.camera_look_at((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), 10.0, W, H, spp, 4)
                scene = hs.view(cam, SUN)
                scene.seed = SEED
                gpu_ctx.upload(scene)
                want, want32, _ = rect.render(scene, W, H)
                assert (want32 == 1.0).all() and (want == 255).all()
                for flags in (0, 16):
                    rgb, f32, _ = gpu_ctx.render_to_host(_desc(dsrt, W, H, spp, 4, tune=(0, 0, 0, flags)), want_f32=True)
                    _same(rgb, f32, want, want32, (hex(xp), spp, flags))
    finally:
        dsrt.set_experiment(0)


def _corner_scene(dsrt):
    """Triangles only, black sky: two small lit plates near the top of the view of a camera at (0, 0, 10) looking at the origin, the
    second catching the first's bounce light."""
    capi = dsrt.capi
    tri = np.zeros(4, capi.TRI_DTYPE)
    quads = [((-0.2, 3.0, 0.0), (0.2, 3.0, 0.0), (0.2, 3.3, 0.0), (-0.2, 3.3, 0.0), (0.0, 0.0, 1.0)),
             ((-0.2, 3.0, 0.0), (0.2, 3.0, 0.0), (0.2, 3.0, 0.4), (-0.2, 3.0, 0.4), (0.0, 1.0, 0.0))]
    k = 0
    for a, b, c, d, n in quads:
        for v in ((a, b, c), (a, c, d)):
            tri["v"][k] = v
            tri["n"][k] = [n] * 3
            k += 1
    tri["albedo_tex"] = -1
    mats = np.zeros(1, capi.MAT_DTYPE)
    mats["albedo"] = (0.8, 0.6, 0.4)
    mats["albedo_tex"] = -1
    hs = dsrt.HostScene().add_arrays(tris=tri, mats=mats)
    hs.build_bvh()
    return hs


def test_subsequence_numbers_above_two_to_the_32(dsrt, gpu_ctx, rect):
    """512 x 512 at 32768 spp: every pixel above the middle row has (x + y*W) * spp >= 2^32, so its sub-sequence has a nonzero high word.
    The geometry sits in a small window near the top; culling removes the rest of the frame, which must come back as zero bytes."""
    hs = _corner_scene(dsrt)
    W, H, spp, depth = 512, 512, 32768, 4
    sun = (0.3, -0.5, -0.8)
    cam = dsrt.camera_look_at((0.0, 0.0, 10.0), (0.0, 0.0, 0.0), 40.0, W, H, spp, depth)
    scene = hs.view(cam, sun)
    scene.seed = SEED
    gpu_ctx.upload(scene)
    rgb, f32, st = gpu_ctx.render_to_host(_desc(dsrt, W, H, spp, depth), want_f32=True)
    assert st.tiles_culled > 0
    lit = np.argwhere(rgb.max(axis=2) > 0)
    assert len(lit) > 20
    (r0, c0), (r1, c1) = lit.min(axis=0), lit.max(axis=0)
    y0, y1 = H - 1 - r1, H - r0                                       # kernel rows (0 = bottom) of the lit window
    assert y0 > H // 2 and (y0 * W) * spp >= 1 << 32                 # the whole window is above 2^32
    x0, x1, y0, y1 = max(0, c0 - 3), min(W, c1 + 4), max(0, y0 - 3), min(H, y1 + 3)
    want, want32, _ = rect.render(scene, W, H, x0=x0, x1=x1, y0=y0, y1=y1)
    _same(rgb[H - y1:H - y0, x0:x1], f32[H - y1:H - y0, x0:x1], want[H - y1:H - y0, x0:x1], want32[H - y1:H - y0, x0:x1], "window")
    outside = np.ones((H, W), bool)
    outside[H - y1:H - y0, x0:x1] = False
    assert not rgb[outside].any() and not f32.view(np.uint32)[outside].any()
    # whole rows: one through the plates, one just above the window, one at the top
    rows = [(y0 + y1) // 2, min(H - 1, y1 + 1), H - 1]
    want_rows, want_rows32, _ = rect.render(scene, W, H, rows=rows)
    for y in rows:
        r = H - 1 - y
        _same(rgb[r], f32[r], want_rows[r], want_rows32[r], f"row {y}")


def test_empty_tile_culling_is_exact_in_mode1(dsrt, gpu_ctx, rect):
    """The four views of test_gpu_parity::test_empty_tile_culling_is_exact: culled or not, whole or in three shards, the oracle's bytes."""
    import torch
    hs = load_world(dsrt, "station_3k")
    uploaded = False
    views = [((-0.7, 0.0, 260.0), (0.0, 0.0, 0.0), 200, 112, True),
             ((60.0, 45.0, 120.0), (30.0, 10.0, 0.0), 157, 83, True),
             ((0.0, 0.0, 300.0), (250.0, 0.0, 0.0), 96, 64, True),
             ((0.5, 0.2, 0.3), (10.0, 0.0, 0.0), 96, 64, False)]
    stream = torch.cuda.current_stream().cuda_stream
    for lookfrom, lookat, W, H, expect_culled in views:
        cam = dsrt.camera_look_at(lookfrom, lookat, 40.0, W, H, 8, 12)
        scene = hs.view(cam, SUN)
        scene.seed = SEED
        if not uploaded:
            gpu_ctx.upload(scene)
            uploaded = True
        else:
            gpu_ctx.set_camera_sun(cam, SUN)
        want, want32, _ = rect.render(scene, W, H)
        rgb, f32, st = gpu_ctx.render_to_host(_desc(dsrt, W, H, 8, 12), want_f32=True)
        assert (st.tiles_culled > 0) == expect_culled, (lookfrom, st.tiles_culled)
        _same(rgb, f32, want, want32, lookfrom)
        rgb, f32, st_all = gpu_ctx.render_to_host(_desc(dsrt, W, H, 8, 12, tune=(0, 0, 0, 2)), want_f32=True)
        assert st_all.tiles_culled == 0
        _same(rgb, f32, want, want32, (lookfrom, "no culling"))
        world, tile = 3, 8
        lay = dsrt.shard_layout(_desc(dsrt, W, H, 8, 12, tile_size=tile, shard_count=world))
        gathered = torch.full((world * lay["rgb8_bytes_padded"],), 77, dtype=torch.uint8, device="cuda")
        for rank in range(world):
            part = gathered[rank * lay["rgb8_bytes_padded"]:(rank + 1) * lay["rgb8_bytes_padded"]]
            gpu_ctx.render(_desc(dsrt, W, H, 8, 12, tile_size=tile, shard_rank=rank, shard_count=world), part.data_ptr(), stream=stream)
        image = torch.zeros(H * W * 3, dtype=torch.uint8, device="cuda")
        gpu_ctx.deinterleave(_desc(dsrt, W, H, 8, 12, tile_size=tile, shard_count=world), gathered.data_ptr(), image.data_ptr(), stream=stream)
        torch.cuda.synchronize()
        _same(image.cpu().numpy().reshape(H, W, 3), None, want, None, (lookfrom, "shards"))


def _shards(dsrt, ctx, desc_of, W, H, world, tile=0):
    import torch
    stream = torch.cuda.current_stream().cuda_stream
    lay = dsrt.shard_layout(desc_of(tile_size=tile, shard_count=world))
    gathered = torch.full((world * lay["rgb8_bytes_padded"],), 9, dtype=torch.uint8, device="cuda")
    for rank in range(world):
        part = gathered[rank * lay["rgb8_bytes_padded"]:(rank + 1) * lay["rgb8_bytes_padded"]]
        ctx.render(desc_of(tile_size=tile, shard_rank=rank, shard_count=world), part.data_ptr(), stream=stream)
    image = torch.zeros(H * W * 3, dtype=torch.uint8, device="cuda")
    ctx.deinterleave(desc_of(tile_size=tile, shard_count=world), gathered.data_ptr(), image.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    return image.cpu().numpy().reshape(H, W, 3)


def test_shards_and_scheduling_switches_match_the_oracle(dsrt, gpu_ctx, rect):
    """Three shards de-interleaved; stealing off; the mode-1 development switches: slices per heavy pixel (bits 8-19), the least length of a
    background item (bits 28-29), background pixels one item each (bit 31)."""
    hs, scene, W, H, spp, depth = _case(dsrt, "station_near", spp=48)
    want, want32, _ = rect.render(scene, W, H)
    gpu_ctx.upload(scene)
    for world, tile in ((3, 8), (2, 16)):
        img = _shards(dsrt, gpu_ctx, lambda **kw: _desc(dsrt, W, H, spp, depth, **kw), W, H, world, tile)
        _same(img, None, want, None, ("shards", world, tile))
    for flags in (16, 1, 2, 4, 1 + 16, 12):
        rgb, f32, _ = gpu_ctx.render_to_host(_desc(dsrt, W, H, spp, depth, tune=(0, 0, 0, flags)), want_f32=True)
        _same(rgb, f32, want, want32, ("flags", flags))
    try:
        for xp in (1 << 8, 3 << 8, 5 << 8, 16 << 8, 48 << 8, 0xFFF << 8, 1 << 28, 2 << 28, 3 << 28, 1 << 31, (1 << 31) | (1 << 8)):
            dsrt.set_experiment(xp)
            for flags in (0, 16):
                rgb, f32, _ = gpu_ctx.render_to_host(_desc(dsrt, W, H, spp, depth, tune=(0, 0, 0, flags)), want_f32=True)
                _same(rgb, f32, want, want32, ("experiment", hex(xp), flags))
    finally:
        dsrt.set_experiment(0)


def _station(dsrt, tmp_path, tris):
    from dsrt_amd import meshgen
    obj = tmp_path / f"iss_{tris}.obj"
    if not obj.exists():
        meshgen.generate(obj, tris)
    hs = dsrt.HostScene().add_obj(obj)
    hs.build_bvh()
    poses = dsrt.read_pose_file(os.path.join(GOLDEN, "rendezvous_1s_dt0_01s.txt"))
    return obj, hs, poses


def test_eight_ranks_at_the_1080p_layout(dsrt, gpu_ctx, rect, tmp_path):
    """1920 x 1080 in 8 shards (and through the library's one-process path with eight ranks on this GPU): the whole-frame render, whose rows
    are the oracle's."""
    _, hs, poses = _station(dsrt, tmp_path, 60000)
    fr = dsrt.pose_to_frame(poses[98])
    W, H, spp, depth, world = 1920, 1080, 2, 50, 8
    cam = dsrt.frame_camera(fr, 40.0, W, H, spp, depth)
    sun = tuple(fr.sun_dir_model)
    scene = hs.view(cam, sun)
    scene.seed = SEED
    gpu_ctx.upload(scene)
    whole, f32, _ = gpu_ctx.render_to_host(_desc(dsrt, W, H, spp, depth), want_f32=True)
    rows = [540, 3, 1076, 777]
    want, want32, _ = rect.render(scene, W, H, rows=rows)
    for y in rows:
        r = H - 1 - y
        _same(whole[r], f32[r], want[r], want32[r], f"row {y}")
    assert (whole.max(axis=2) > 0).mean() > 0.2
    img = _shards(dsrt, gpu_ctx, lambda **kw: _desc(dsrt, W, H, spp, depth, **kw), W, H, world)
    _same(img, None, whole, None, "8 shards")
    multi = dsrt.Multi([0] * world)
    multi.upload(scene)
    img, _, _ = multi.render_frame(_desc(dsrt, W, H, spp, depth), cam, sun)
    multi.close()
    _same(img, None, whole, None, "Multi, 8 ranks")


def test_batches_and_the_frame_pipeline_match_the_oracle(dsrt, gpu_ctx, rect, tmp_path):
    """dsrt_render_batch with a different camera and sun per frame, whole and in three shards, and sequence.render_frames (4 frames in
    flight): every frame is the oracle's."""
    import torch
    from dsrt_amd import sequence
    _, hs, poses = _station(dsrt, tmp_path, 20000)
    W, H, spp, depth = 150, 85, 24, 50
    frames = [0, 70, 90, 98]

    def frame(i):
        fr = dsrt.pose_to_frame(poses[i])
        return dsrt.frame_camera(fr, 40.0, W, H, spp, depth), tuple(fr.sun_dir_model)
    cams, suns = zip(*[frame(i) for i in frames])
    want = {}
    for k, i in enumerate(frames):
        v = hs.view(cams[k], suns[k])
        v.seed = SEED
        want[i] = rect.render(v, W, H)[:2]
    assert want[98][0].max() > 0
    gpu_ctx.upload(hs.view(cams[0], suns[0]))
    n = len(frames)
    stream = torch.cuda.current_stream().cuda_stream
    rgb = torch.zeros(n * H * W * 3, dtype=torch.uint8, device="cuda")
    f32 = torch.zeros(n * H * W * 3, dtype=torch.float32, device="cuda")
    gpu_ctx.render_batch(_desc(dsrt, W, H, spp, depth), list(cams), list(suns), rgb.data_ptr(), f32.data_ptr(), stream=stream, want_stats=True)
    got, got32 = rgb.cpu().numpy().reshape(n, H, W, 3), f32.cpu().numpy().reshape(n, H, W, 3)
    for k, i in enumerate(frames):
        _same(got[k], got32[k], want[i][0], want[i][1], f"batch, frame {i}")
    world = 3
    lay = dsrt.shard_layout(_desc(dsrt, W, H, spp, depth, shard_count=world))
    pb = lay["rgb8_bytes_padded"]
    parts = []
    for r in range(world):
        buf = torch.zeros(n * pb, dtype=torch.uint8, device="cuda")
        gpu_ctx.render_batch(_desc(dsrt, W, H, spp, depth, shard_rank=r, shard_count=world), list(cams), list(suns), buf.data_ptr(), stream=stream, want_stats=True)
        parts.append(buf)
    for k, i in enumerate(frames):
        gathered = torch.cat([p[k * pb:(k + 1) * pb] for p in parts])
        image = torch.zeros(W * H * 3, dtype=torch.uint8, device="cuda")
        gpu_ctx.deinterleave(_desc(dsrt, W, H, spp, depth, shard_count=world), gathered.data_ptr(), image.data_ptr(), stream=stream)
        torch.cuda.synchronize()
        _same(image.cpu().numpy().reshape(H, W, 3), None, want[i][0], None, f"sharded batch, frame {i}")
    # the frame pipeline describes its frames with make_desc's default seed
    seq_want = {}
    for k, i in enumerate(frames):
        v = hs.view(cams[k], suns[k])
        v.seed = 1337
        seq_want[i] = rect.render(v, W, H)[0]
    got = sequence.render_frames(dsrt, gpu_ctx, frame, frames, W, H, spp, depth, inflight=4, rng_mode=1)
    assert sorted(got) == frames
    for i in frames:
        _same(got[i], None, seq_want[i], None, f"render_frames, frame {i}")


def test_certified_tree_matches_the_oracle(dsrt, rect):
    ctx = dsrt.Context(0).set_certified_tree(True)
    try:
        for name in ("station_near", "mixed"):
            hs, scene, W, H, spp, depth, want, want32, _ = _case_want(dsrt, rect, name)
            ctx.upload(scene)
            rgb, f32, st = ctx.render_to_host(_desc(dsrt, W, H, spp, depth), want_f32=True)
            assert st.certified_tree_used == 1, name
            _same(rgb, f32, want, want32, name)
            rgb, f32, st = ctx.render_to_host(_desc(dsrt, W, H, spp, depth, collect_counters=3), want_f32=True)
            assert st.certificate_audit_mismatches == 0
            _same(rgb, f32, want, want32, (name, "audit"))
    finally:
        ctx.close()


@pytest.mark.parametrize("kind", ["sah", "lbvh"])
def test_fast_trees_match_the_oracle_on_that_tree(dsrt, gpu_ctx, rect, kind):
    world, cam_args, spp = CASES["station_near"]
    hs = load_world(dsrt, world)
    hs.build_bvh(kind)
    W, H, depth = cam_args[3], cam_args[4], cam_args[5]
    scene = hs.view(dsrt.camera_look_at(cam_args[0], cam_args[1], cam_args[2], W, H, spp, depth), SUN)
    scene.seed = SEED
    want, want32, _ = rect.render(scene, W, H)
    gpu_ctx.upload(scene)
    rgb, f32, _ = gpu_ctx.render_to_host(_desc(dsrt, W, H, spp, depth), want_f32=True)
    _same(rgb, f32, want, want32, kind)


def test_widest_image_the_pixel_packing_allows(dsrt, gpu_ctx, rect):
    """Samples change lanes with 16-bit pixel coordinates: width 65535 renders the oracle's bytes, width 65536 is refused."""
    hs = load_world(dsrt, "lights")
    W, H, spp = 65535, 2, 3
    cam = dsrt.camera_look_at((0.0, 3.0, 9.0), (0.0, 2.0, 0.0), 45.0, W, H, spp, 12)
    scene = hs.view(cam, SUN)
    scene.seed = SEED
    gpu_ctx.upload(scene)
    want, want32, _ = rect.render(scene, W, H)
    assert want.max() > 0
    for flags in (0, 16):
        rgb, f32, _ = gpu_ctx.render_to_host(_desc(dsrt, W, H, spp, 12, tune=(0, 0, 0, flags)), want_f32=True)
        _same(rgb, f32, want, want32, ("width 65535", flags))
    cam = dsrt.camera_look_at((0.0, 3.0, 9.0), (0.0, 2.0, 0.0), 45.0, W + 1, H, spp, 12)
    gpu_ctx.set_camera_sun(cam, SUN)
    with pytest.raises(dsrt.DsrtError):
        gpu_ctx.render_to_host(_desc(dsrt, W + 1, H, spp, 12))


# math_mode 1 (the device's own sinf / cosf / powf) has no CPU counterpart: its rng_mode 1 image lies this close to the oracle's.  Measured on
# an MI355X over the six parity scenes (at the seed above): largest mean absolute difference of the float image 3.2e-09 (c1_spheres), largest
# pixel difference 2.3e-06 (lights): rounding-sized, far below what one sample taking another branch would leave at these sample counts.  The
# max bound leaves room for a few such flips; the mean bound is five orders of magnitude tighter than the 0.03 of the comparison with mode 0.
MATH1_MEAN_ABS = 1e-7
MATH1_MAX_ABS = 1e-3


def test_math_mode1_stays_close_to_the_oracle(dsrt, gpu_ctx, rect):
    worst_mean = worst_max = 0.0
    for name in sorted(CASES):
        hs, scene, W, H, spp, depth, want, want32, _ = _case_want(dsrt, rect, name)
        gpu_ctx.upload(scene)
        rgb, f32, _ = gpu_ctx.render_to_host(_desc(dsrt, W, H, spp, depth, math_mode=1), want_f32=True)
        d = np.abs(f32.astype(np.float64) - want32.astype(np.float64))
        worst_mean, worst_max = max(worst_mean, float(d.mean())), max(worst_max, float(d.max()))
        print(f"math_mode 1 vs oracle, {name}: mean |d| {d.mean():.3e}, max |d| {d.max():.3e}, pixels differing {(d.max(axis=2) > 0).mean():.4f}")
    print(f"math_mode 1 vs oracle: worst mean |d| {worst_mean:.3e}, worst max |d| {worst_max:.3e}")
    assert worst_mean < MATH1_MEAN_ABS and worst_max < MATH1_MAX_ABS, (worst_mean, worst_max)
