"""Masked accumulate launches where the list of active pixels is built differently (render_kernel.hip, dsrt_pixel_count/scan/list_kernel): tiles of more than one
8x8 block, and frames whose tiles outnumber the scan's 1024 threads or leave most of them idle; and Accumulator's `+=` refusing per-pixel counts before it has
added anything.  Bit patterns, sentinels and helpers are tests/test_gpu_adaptive.py's."""
import numpy as np
import pytest

from _sample_sets import parity_case
from test_gpu_adaptive import SEED, _check_mask, _desc, _station, _unmasked

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("tile", [16, 32])
def test_masks_on_tiles_of_several_blocks(dsrt, gpu_ctx, tile):
    """tile_size 16 and 32: four and sixteen 8x8 blocks per tile, on a frame (97 x 61) that is a multiple of neither -- blocks wholly and partly outside it."""
    W, H, spp = 97, 61, 8
    hs, scene = _station(dsrt, W, H, spp)
    gpu_ctx.upload(scene)
    split = [(1, 3, 2)]
    R, R2 = _unmasked(dsrt, gpu_ctx, _desc(dsrt, W, H, spp, 50), split)             # the sums do not depend on the tiling
    assert R.any()
    desc = _desc(dsrt, W, H, spp, 50, tile_size=tile)
    Rt, Rt2 = _unmasked(dsrt, gpu_ctx, desc, split)
    assert np.array_equal(Rt, R) and np.array_equal(Rt2, R2)
    bern = (np.random.default_rng(11).random((H, W)) < 0.3).astype(np.uint8)
    edge = np.zeros((H, W), np.uint8)
    edge[:, W - 1] = 1
    edge[H - 1, :] = 1
    for what, mask in (("Bernoulli(0.3)", bern), ("last column and row", edge), ("all ones", np.ones((H, W), np.uint8)), ("empty", np.zeros((H, W), np.uint8))):
        _check_mask(dsrt, gpu_ctx, desc, split, mask, R, R2, (tile, what))
    _check_mask(dsrt, gpu_ctx, _desc(dsrt, W, H, spp, 50, tile_size=tile, tune=(0, 0, 0, 2)), split, bern, R, R2, (tile, "Bernoulli, no culling"))


def test_masks_on_a_frame_of_more_blocks_than_the_scan_has_threads(dsrt, gpu_ctx):
    """320 x 240 at the default tile: 1200 blocks, so the 1024 threads of the prefix sum hold two each and the last ones none; 4 samples of depth 4 keep it quick."""
    W, H, spp = 320, 240, 4
    hs, scene = _station(dsrt, W, H, spp)
    gpu_ctx.upload(scene)
    desc = _desc(dsrt, W, H, spp, 4)
    split = [(0, 2, 2)]
    R, R2 = _unmasked(dsrt, gpu_ctx, desc, split)
    assert R.any()
    bern = (np.random.default_rng(13).random((H, W)) < 0.3).astype(np.uint8)
    _check_mask(dsrt, gpu_ctx, desc, split, bern, R, R2, "Bernoulli(0.3)")
    _check_mask(dsrt, gpu_ctx, _desc(dsrt, W, H, spp, 4, tune=(0, 0, 0, 2)), split, bern, R, R2, "Bernoulli(0.3), no culling")
    _check_mask(dsrt, gpu_ctx, desc, split, np.ones((H, W), np.uint8), R, R2, "all ones")


def test_a_refused_add_of_accumulators_leaves_the_sums_alone(dsrt, gpu_ctx):
    hs, scene, W, H, spp, depth = parity_case(dsrt, "lights", SEED)
    gpu_ctx.upload(scene)
    desc = _desc(dsrt, W, H, spp, depth)
    a, b = dsrt.Accumulator(gpu_ctx, desc, moments=True), dsrt.Accumulator(gpu_ctx, desc, moments=True)
    a.render(0, 2)
    b.render(2, 2)
    torch.cuda.synchronize()
    assert b.sum.any() and b.sum_sq.any()
    s, sq = a.sum.clone(), a.sum_sq.clone()
    for other in (dsrt.Accumulator(gpu_ctx, desc, moments=True, counts=True), None):
        if other is None:                                    # an accumulator that holds a masked set
            other = b
            other.render(4, 1, mask=torch.ones(W * H, dtype=torch.uint8, device=a.sum.device))
        else:
            other.render(2, 2)
        with pytest.raises(ValueError):
            a += other
        assert torch.equal(a.sum, s) and torch.equal(a.sum_sq, sq) and a.samples_done == 2 and a.n is None
    c = dsrt.Accumulator(gpu_ctx, desc, moments=True, counts=True)      # ... and the left side with counts refuses too, unchanged
    c.render(0, 2)
    s, sq = c.sum.clone(), c.sum_sq.clone()
    d = dsrt.Accumulator(gpu_ctx, desc, moments=True)
    d.render(2, 2)
    with pytest.raises(ValueError):
        c += d
    assert torch.equal(c.sum, s) and torch.equal(c.sum_sq, sq)
