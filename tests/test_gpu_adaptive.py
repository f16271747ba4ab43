"""Adaptive sampling on the GPU (include/dsrt.h, ADAPTIVE SAMPLING): a masked accumulate launch adds to the active pixels exactly what the unmasked launch adds
and leaves every other word alone, the convergence test is the numpy model's byte for byte, the per-pixel resolve is the CPU resolve of every pixel's own
count, the driver is the loop over the three primitives, every refusal is a refusal, and the CLI.  Bit patterns are compared throughout; wherever "adds" and
"untouched" matter the buffers start from a nonzero sentinel."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ASSETS, GOLDEN, ROOT, load_world
from test_oracle import CASES, SUN
from _sample_sets import SetOracle, interleaved, parity_case
from _adaptive_model import UINT32_MAX, converged, needed_tolerance, select_unconverged
from test_adaptive_host import SETTINGS, edge_pixels

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

SEED = 0xDEADBEEF00001337
DEV = "cuda:0"
VARIANTS = [{}, {"math_mode": 1}, {"checked": 1}, {"tune": (0, 0, 0, 2)}, {"tune": (0, 0, 0, 16)}]


@pytest.fixture(scope="module")
def sets(dsrt):
    return SetOracle()


@pytest.fixture(scope="module")
def cert_ctx(dsrt):
    ctx = dsrt.Context(0).set_certified_tree(True)
    yield ctx
    ctx.close()


def _desc(dsrt, W, H, spp, depth, **kw):
    return dsrt.make_desc(W, H, spp, depth, seed=SEED, rng_mode=1, **kw)


def _u64(t, shape):
    return t.cpu().numpy().view(np.uint64).reshape(shape)


def _dev64(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).reshape(-1).view(np.int64)).to(DEV)


def _dev32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).to(DEV)


def _sentinels(W, H):
    """Nonzero starting words for sum, sum_sq (uint64 (H, W, 3)) and n (uint32 (H, W))."""
    i = np.arange(W * H * 3, dtype=np.uint64).reshape(H, W, 3)
    return i * np.uint64(7) + np.uint64(3), i * np.uint64(11) + np.uint64(5), (np.arange(W * H, dtype=np.uint32) % 1000 + 5).reshape(H, W)


def _unmasked(dsrt, ctx, desc, split):
    """(R, R2) uint64 (H, W, 3): what the unmasked launches of `split` add to zeroed sums."""
    acc = dsrt.Accumulator(ctx, desc, moments=True)
    for first, count, stride in split:
        acc.render(first, count, stride)
    torch.cuda.synchronize()
    shape = (desc.height, desc.width, 3)
    return _u64(acc.sum, shape), _u64(acc.sum_sq, shape)


def _masked(ctx, desc, split, mask, s0, sq0, n0):
    """The masked launches of `split` on buffers that start at (s0, sq0, n0): the buffers afterwards."""
    s, sq, n, m = _dev64(s0), _dev64(sq0), _dev32(n0), torch.from_numpy(np.ascontiguousarray(mask, np.uint8)).to(DEV)
    for first, count, stride in split:
        ctx.render_accumulate_masked(desc, first, count, stride, s, sq, m, n)
    torch.cuda.synchronize()
    H, W = desc.height, desc.width
    return _u64(s, (H, W, 3)), _u64(sq, (H, W, 3)), n.cpu().numpy().view(np.uint32).reshape(H, W)


def _check_mask(dsrt, ctx, desc, split, mask, R, R2, what):
    """Active pixels: sentinel + the unmasked launch's words; every other word: the sentinel."""
    H, W = desc.height, desc.width
    s0, sq0, n0 = _sentinels(W, H)
    got, got2, gotn = _masked(ctx, desc, split, mask, s0, sq0, n0)
    on = (np.asarray(mask) != 0)
    total = np.uint32(sum(c for _, c, _ in split))
    assert np.array_equal(got, s0 + R * on[..., None].astype(np.uint64)), (what, "sum")
    assert np.array_equal(got2, sq0 + R2 * on[..., None].astype(np.uint64)), (what, "sum_sq")
    assert np.array_equal(gotn, n0 + total * on.astype(np.uint32)), (what, "n")


# ---- 1. an all-ones mask is the unmasked launch ----
@pytest.mark.parametrize("name", sorted(CASES))
def test_all_ones_mask_is_the_unmasked_launch(dsrt, gpu_ctx, cert_ctx, name):
    hs, scene, W, H, spp, depth = parity_case(dsrt, name, SEED)
    ones = np.ones((H, W), np.uint8)
    for ctx in (gpu_ctx, cert_ctx):
        ctx.upload(scene)
        for split in ([(1, 3, 2)], interleaved(spp, 4)[:2]):
            for kw in VARIANTS:
                desc = _desc(dsrt, W, H, spp, depth, **kw)
                R, R2 = _unmasked(dsrt, ctx, desc, split)
                assert R.any() and R2.any()
                got, got2, gotn = _masked(ctx, desc, split, ones, np.zeros_like(R), np.zeros_like(R2), np.zeros((H, W), np.uint32))
                what = (name, ctx is cert_ctx, split, kw)
                assert np.array_equal(got, R), (what, "sum")
                assert np.array_equal(got2, R2), (what, "sum_sq")
                assert (gotn == sum(c for _, c, _ in split)).all(), (what, "n")
                # without second moments and without counts: the other kernel, the same sums
                s = torch.zeros(W * H * 3, dtype=torch.int64, device=DEV)
                for first, count, stride in split:
                    ctx.render_accumulate_masked(desc, first, count, stride, s, None, torch.from_numpy(ones).to(DEV), None)
                torch.cuda.synchronize()
                assert np.array_equal(_u64(s, (H, W, 3)), R), (what, "sum, no moments")


# ---- 2. masks that can go wrong ----
def _station(dsrt, W, H, spp, lookfrom=(12.0, 9.0, 38.0)):
    hs = load_world(dsrt, "station_3k")
    scene = hs.view(dsrt.camera_look_at(lookfrom, (0.0, 0.0, 0.0), 40.0, W, H, spp, 50), SUN)
    scene.seed = SEED
    return hs, scene


def test_masks_that_can_go_wrong(dsrt, gpu_ctx, sets):
    hs, scene, W, H, spp, depth = parity_case(dsrt, "station_near", SEED)
    gpu_ctx.upload(scene)
    desc = _desc(dsrt, W, H, spp, depth)
    split = [(1, 3, 2)]
    R, R2 = _unmasked(dsrt, gpu_ctx, desc, split)
    z = lambda: np.zeros((H, W), np.uint8)          # noqa: E731
    masks = {"empty": z()}
    m = z(); m[H - 1, 0] = 1; masks["bottom-left (kernel y = 0)"] = m
    m = z(); m[0, W - 1] = 1; masks["top-right"] = m
    m = z(); m[3::8, 5::8] = 1; masks["one pixel in every 8x8 tile"] = m
    m = z(); m[48:56, 96:104] = 1; masks["one whole tile"] = m
    m = z(); m[48:56, 96:104] = 255; m[10, 10] = 128; masks["bytes of 255 and 128"] = m
    bern = (np.random.default_rng(7).random((H, W)) < 0.3).astype(np.uint8)
    masks["Bernoulli(0.3)"] = bern
    assert R[48:56, 96:104].any() and bern.any() and not bern.all()
    for what, mask in masks.items():
        _check_mask(dsrt, gpu_ctx, desc, split, mask, R, R2, what)
    # the checked kernel, no culling, natural order (no pre-pass order at all)
    for kw in ({"checked": 1}, {"tune": (0, 0, 0, 2)}, {"tune": (0, 0, 0, 1)}):
        _check_mask(dsrt, gpu_ctx, _desc(dsrt, W, H, spp, depth, **kw), split, bern, R, R2, ("Bernoulli", kw))
    # on a 24 x 16 rectangle the active pixels are the CPU model's
    box = dict(x0=W // 2 - 12, x1=W // 2 + 12, y0=H // 2 - 8, y1=H // 2 + 8)
    S, S2 = sets.sums(scene, W, H, 1, 3, 2, **box)
    r0, r1, c0, c1 = H - box["y1"], H - box["y0"], box["x0"], box["x1"]
    on = bern[r0:r1, c0:c1] != 0
    assert on.any() and S[r0:r1, c0:c1][on].any()
    got, got2, _ = _masked(gpu_ctx, desc, split, bern, np.zeros_like(R), np.zeros_like(R2), np.zeros((H, W), np.uint32))
    assert np.array_equal(got[r0:r1, c0:c1][on], S[r0:r1, c0:c1][on]) and np.array_equal(got2[r0:r1, c0:c1][on], S2[r0:r1, c0:c1][on])
    assert not got[r0:r1, c0:c1][~on].any()


def test_last_column_and_row_of_a_frame_that_is_no_multiple_of_the_tile(dsrt, gpu_ctx):
    W, H, spp = 97, 61, 8
    hs, scene = _station(dsrt, W, H, spp)
    gpu_ctx.upload(scene)
    desc = _desc(dsrt, W, H, spp, 50)
    split = [(0, 3, 2), (5, 1, 1)]
    R, R2 = _unmasked(dsrt, gpu_ctx, desc, split)
    mask = np.zeros((H, W), np.uint8)
    mask[:, W - 1] = 1
    mask[H - 1, :] = 1
    _check_mask(dsrt, gpu_ctx, desc, split, mask, R, R2, "last column and row")
    mask = np.zeros((H, W), np.uint8)
    mask[H // 2, :] = 1                                    # a row through the geometry, edge pixel included
    assert R[H // 2].any()
    _check_mask(dsrt, gpu_ctx, desc, split, mask, R, R2, "middle row")
    _check_mask(dsrt, gpu_ctx, desc, split, np.ones((H, W), np.uint8), R, R2, "all ones")


def test_mask_inside_culled_tiles_moves_only_the_counts(dsrt, gpu_ctx):
    hs, scene, W, H, spp, depth = parity_case(dsrt, "station_far", SEED)
    gpu_ctx.upload(scene)
    desc = _desc(dsrt, W, H, spp, depth)
    st = dsrt.Accumulator(gpu_ctx, desc).render(0, 2, want_stats=True)
    assert st.tiles_culled > 0                               # the far station: the pre-pass removes provably empty tiles
    R, R2 = _unmasked(dsrt, gpu_ctx, desc, [(1, 3, 2)])
    lit = np.argwhere(R.max(axis=2) > 0)
    assert len(lit) and lit[:, 0].min() > 24 and lit[:, 1].min() > 24         # nothing anywhere near the top-left corner ...
    mask = np.zeros((H, W), np.uint8)
    mask[0:16, 0:16] = 1                                                         # ... whose four tiles the pre-pass culls
    s0, sq0, n0 = _sentinels(W, H)
    got, got2, gotn = _masked(gpu_ctx, desc, [(1, 3, 2)], mask, s0, sq0, n0)
    assert np.array_equal(got, s0) and np.array_equal(got2, sq0)
    assert np.array_equal(gotn, n0 + np.uint32(3) * mask.astype(np.uint32))


def test_one_pixel_with_more_samples_than_an_item_holds(dsrt, gpu_ctx):
    """spp = count = 4100: past the 4095 samples a work item's 32-bit sums hold, so the one active pixel is cut whatever its tile sees."""
    hs, scene, W, H, _, depth = parity_case(dsrt, "lights", SEED, 4100)
    gpu_ctx.upload(scene)
    desc = _desc(dsrt, W, H, 4100, depth)
    split = [(0, 4100, 1)]
    R, R2 = _unmasked(dsrt, gpu_ctx, desc, split)
    for r, c in ((H // 2, W // 2), (1, 1)):                  # a pixel that sees the scene and one near the corner
        mask = np.zeros((H, W), np.uint8)
        mask[r, c] = 1
        _check_mask(dsrt, gpu_ctx, desc, split, mask, R, R2, ("4100 samples", r, c))
    assert R[H // 2, W // 2].any()


# ---- 3. the convergence test is the numpy model ----
def _select(ctx, desc, S, S2, n, tol, floor, n_min=0, n_max=UINT32_MAX):
    mask, active = ctx.select_unconverged(desc, _dev64(S), _dev64(S2), _dev32(n), tol, floor, n_min, n_max)
    torch.cuda.synchronize()
    return mask.cpu().numpy(), active


@pytest.mark.parametrize("name", sorted(CASES))
def test_select_unconverged_on_the_gpus_own_sums(dsrt, gpu_ctx, name):
    hs, scene, W, H, spp, depth = parity_case(dsrt, name, SEED)
    gpu_ctx.upload(scene)
    desc = _desc(dsrt, W, H, spp, depth)
    acc = dsrt.Accumulator(gpu_ctx, desc, moments=True, counts=True)
    for first, count, stride in interleaved(spp, 4)[:2]:
        acc.render(first, count, stride)
    torch.cuda.synchronize()
    S, S2 = _u64(acc.sum, (H, W, 3)), _u64(acc.sum_sq, (H, W, 3))
    n = acc.n.cpu().numpy().view(np.uint32)
    assert (n == sum(c for _, c, _ in interleaved(spp, 4)[:2])).all()
    seen = set()
    for tol, floor, n_min, n_max in [(0.05, 0.0, 0, UINT32_MAX), (0.3, 0.01, 0, UINT32_MAX), (0.0, 0.0, 0, UINT32_MAX), (1e30, 0.0, 0, UINT32_MAX), (0.3, 0.0, 0, 4)]:
        want = select_unconverged(S, S2, n, tol, floor, n_min, n_max)
        mask, active = acc.ctx.select_unconverged(desc, acc.sum, acc.sum_sq, acc.n, tol, floor, n_min, n_max)
        torch.cuda.synchronize()
        assert np.array_equal(mask.cpu().numpy(), want), (name, tol, floor, (mask.cpu().numpy() != want).sum())
        assert active == int(want.sum())
        seen.update(np.unique(want).tolist())
    assert seen == {0, 1}, name


def test_select_unconverged_on_hand_made_sums(dsrt, gpu_ctx):
    S, S2, n, what = edge_pixels()
    W, H = 16, 8                                             # the edge pixels first, then random ones
    rng = np.random.default_rng(11)
    k = len(n)
    Sf = rng.integers(0, 6 << 20, size=(W * H, 3)).astype(np.uint64)
    nf = rng.integers(0, 12, size=W * H).astype(np.uint32)
    S2f = (Sf.astype(np.float64) ** 2 / np.maximum(nf, 1)[:, None] / 2.0 ** 20 * rng.uniform(0.9, 1.3, size=(W * H, 3))).astype(np.uint64)
    Sf[:k], S2f[:k], nf[:k] = S, S2, n
    Sf, S2f, nf = Sf.reshape(H, W, 3), S2f.reshape(H, W, 3), nf.reshape(H, W)
    desc = _desc(dsrt, W, H, 16, 4)
    for tol, floor, n_min, n_max in SETTINGS:
        want = select_unconverged(Sf, S2f, nf, tol, floor, n_min, n_max)
        got, active = _select(gpu_ctx, desc, Sf, S2f, nf, tol, floor, n_min, n_max)
        bad = np.flatnonzero((got != want).reshape(-1))
        assert not bad.size, (tol, floor, n_min, n_max, [what[i] if i < k else int(i) for i in bad])
        assert active == int(want.sum())
    # the exact-limit pixel is converged on the GPU too, its neighbour one unit past the limit is not
    got, _ = _select(gpu_ctx, desc, Sf, S2f, nf, 0.5, 0.0)
    flat = got.reshape(-1)
    assert flat[what.index("vm == lim*lim exactly (rel_tol 0.5, floor 0)")] == 0 and flat[what.index("one unit past the limit")] == 1
    # without want_active the call does not synchronise and returns no count
    mask, active = gpu_ctx.select_unconverged(desc, _dev64(Sf), _dev64(S2f), _dev32(nf), 0.5, 0.0, want_active=False)
    torch.cuda.synchronize()
    assert active is None and np.array_equal(mask.cpu().numpy(), got)


# ---- 4. the per-pixel resolve is the CPU resolve of every pixel's own count ----
def _check_resolve_counts(ctx, sets, desc, S, S2, n, gamma, what):
    rgb, f32, var = ctx.resolve_accumulated_counts(desc, _dev64(S), _dev32(n), _dev64(S2), want_f32=True, want_var=True)
    torch.cuda.synchronize()
    rgb, f32, var = rgb.cpu().numpy(), f32.cpu().numpy(), var.cpu().numpy()
    for cnt in np.unique(n):
        at = n == cnt
        if cnt == 0:
            assert not rgb[at].any() and not f32[at].view(np.uint32).any() and not var[at].view(np.uint32).any(), (what, "n = 0")
            continue
        w_rgb, w_f32, w_var = sets.resolve(S[at], S2[at], int(cnt), gamma, want_var=cnt >= 2)
        assert np.array_equal(rgb[at], w_rgb), (what, int(cnt), "rgb8")
        assert np.array_equal(f32[at].view(np.uint32), w_f32.view(np.uint32)), (what, int(cnt), "f32")
        if cnt >= 2:
            assert np.array_equal(var[at].view(np.uint32), w_var.view(np.uint32)), (what, int(cnt), "variance")
        else:
            assert not var[at].view(np.uint32).any(), (what, "n = 1: +0.0f")


def test_resolve_accumulated_counts_is_the_cpu_resolve_per_count(dsrt, gpu_ctx, sets):
    hs, scene, W, H, spp, depth = parity_case(dsrt, "station_near", SEED)
    gpu_ctx.upload(scene)
    rng = np.random.default_rng(5)
    for kw in ({}, {"math_mode": 1}):
        desc = _desc(dsrt, W, H, spp, depth, **kw)
        acc = dsrt.Accumulator(gpu_ctx, desc, moments=True, counts=True)
        acc.render(0, 1, 1, mask=torch.from_numpy((rng.random((H, W)) < 0.8).astype(np.uint8)).to(DEV))          # n = 0 and n = 1 pixels
        for p in (1, 2, 3):
            acc.render(p, 3, 4, mask=torch.from_numpy((rng.random((H, W)) < 0.5).astype(np.uint8)).to(DEV))
        torch.cuda.synchronize()
        S, S2, n = _u64(acc.sum, (H, W, 3)), _u64(acc.sum_sq, (H, W, 3)), acc.n.cpu().numpy().view(np.uint32)
        assert {0, 1, 3, 4, 6, 7, 9, 10} <= set(np.unique(n).tolist())
        if not kw:
            _check_resolve_counts(gpu_ctx, sets, desc, S, S2, n, scene.params.gamma, "GPU sums")
        else:
            # the device math library's pow is not the CPU oracle's: with it the per-pixel resolve is held to the uniform resolve of the same library
            rgb, f32, var = acc.resolve_counts(want_f32=True, want_var=True)
            for cnt in (3, 7):
                u_rgb, u_f32, u_var = gpu_ctx.resolve_accumulated(desc, acc.sum, cnt, acc.sum_sq, want_f32=True, want_var=True)
                torch.cuda.synchronize()
                at = torch.from_numpy(n == cnt).to(DEV)
                assert torch.equal(rgb[at], u_rgb[at]) and torch.equal(f32[at].view(torch.int32), u_f32[at].view(torch.int32))
                assert torch.equal(var[at].view(torch.int32), u_var[at].view(torch.int32))
    # hand-made sums: n = 0 with zero sums, n = 1, and the edge pixels of the convergence test
    S, S2, n, _ = edge_pixels()
    Wm, Hm = 4, 3
    assert len(n) == Wm * Hm
    _check_resolve_counts(gpu_ctx, sets, _desc(dsrt, Wm, Hm, 16, 4), S.reshape(Hm, Wm, 3), S2.reshape(Hm, Wm, 3), n.reshape(Hm, Wm), 2.0, "hand-made")


# ---- 5. the driver is the loop over the primitives ----
def _loop(dsrt, ctx, desc, tol, P, M, floor=0.0):
    """dsrt_render_adaptive written with the three calls (include/dsrt.h)."""
    acc = dsrt.Accumulator(ctx, desc, moments=True, counts=True)
    active, per_pass, total, mask = desc.width * desc.height, [], 0, None
    for p in range(P):
        if not active:
            break
        count = len(range(p, desc.spp, P))
        acc.render(p, count, P, mask=None if p < M else mask)
        per_pass.append(active)
        total += active * count
        if M <= p + 1 < P:
            mask, active = ctx.select_unconverged(desc, acc.sum, acc.sum_sq, acc.n, tol, floor)
    images = acc.resolve_counts(want_f32=True, want_var=True)
    torch.cuda.synchronize()
    return acc, images, {"passes_run": len(per_pass), "samples_total": total, "active": per_pass}


def _same_run(a, b, what):
    (acc_a, img_a, st_a), (acc_b, img_b, st_b) = a, b
    assert st_a == st_b, (what, st_a, st_b)
    assert torch.equal(acc_a.sum, acc_b.sum) and torch.equal(acc_a.sum_sq, acc_b.sum_sq) and torch.equal(acc_a.n, acc_b.n), what
    for x, y in zip(img_a, img_b):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), what


@pytest.mark.parametrize("name", ["station_near", "mixed", "station_far"])
def test_driver_is_the_loop_over_the_primitives(dsrt, gpu_ctx, name):
    hs, scene, W, H, spp, depth = parity_case(dsrt, name, SEED)
    gpu_ctx.upload(scene)
    desc = _desc(dsrt, W, H, spp, depth)
    want_rgb, want_f32, _ = gpu_ctx.render_to_host(desc, want_f32=True)
    P = 4
    counts = [len(range(p, spp, P)) for p in range(P)]
    for tol, M in ((0.0, 2), (0.0, P), (1e30, 2), (1e30, 1), (0.05, 1), (0.2, 3)):
        drv = gpu_ctx.render_adaptive(desc, tol, passes=P, min_passes=M, want_f32=True, want_var=True)
        torch.cuda.synchronize()
        _same_run(drv, _loop(dsrt, gpu_ctx, desc, tol, P, M), (name, tol, M))
        acc, (rgb, f32, var), st = drv
        n = acc.n.cpu().numpy()
        assert st["active"][:M] == [W * H] * M and st["samples_total"] == int(n.sum())
        assert all(a >= b for a, b in zip(st["active"], st["active"][1:]))
        assert set(np.unique(n).tolist()) <= {sum(counts[:k]) for k in range(M, P + 1)}           # every count is a prefix sum of the pass counts
        full = n == spp
        if tol == 0.0:
            # every pixel with any variance runs all passes; wherever n == spp the image is dsrt_render's
            assert st["passes_run"] == P and full.any()
            assert np.array_equal(rgb.cpu().numpy()[full], want_rgb[full]) and np.array_equal(f32.cpu().numpy()[full].view(np.uint32), want_f32[full].view(np.uint32))
            if M == P:
                assert full.all()
            else:
                S, S2 = _u64(acc.sum, (H, W, 3)), _u64(acc.sum_sq, (H, W, 3))
                assert converged(S[~full], S2[~full], n[~full].astype(np.uint32), 0.0, 0.0).all()   # the pixels that stopped have no variance at all
        if tol == 1e30:
            assert st["passes_run"] == M and (n == sum(counts[:M])).all()


def test_an_intermediate_tolerance_stops_some_pixels_early_and_not_others(dsrt, gpu_ctx, sets):
    hs, scene, W, H, spp, depth = parity_case(dsrt, "station_near", SEED)
    gpu_ctx.upload(scene)
    desc = _desc(dsrt, W, H, spp, depth)
    P, M = 4, 2
    counts = [len(range(p, spp, P)) for p in range(P)]
    # The tolerance is chosen on the CPU: the set oracle's sums after 2 and after 3 passes over a 24 x 16 rectangle say, for every pixel, below which
    # tolerance it runs to the end (not converged at either test); a tolerance in the widest gap between two such values splits the rectangle's pixels.
    box = dict(x0=W // 2 - 12, x1=W // 2 + 12, y0=H // 2 - 8, y1=H // 2 + 8)
    r0, r1, c0, c1 = H - box["y1"], H - box["y0"], box["x0"], box["x1"]
    S, S2 = np.zeros((H, W, 3), np.uint64), np.zeros((H, W, 3), np.uint64)
    after = {}
    for p in range(P - 1):
        a, a2 = sets.sums(scene, W, H, p, counts[p], P, **box)
        S += a
        S2 += a2
        after[p + 1] = (S[r0:r1, c0:c1].copy(), S2[r0:r1, c0:c1].copy())
    cnt = lambda k: np.full((r1 - r0, c1 - c0), sum(counts[:k]), np.uint32)          # noqa: E731
    runs_below = np.minimum(needed_tolerance(*after[2], cnt(2), 0.0), needed_tolerance(*after[3], cnt(3), 0.0))
    vals = np.unique(runs_below[runs_below > 0])
    assert len(vals) > 8
    mid = vals[len(vals) // 4: 3 * len(vals) // 4 + 1]
    g = int(np.argmax(mid[1:] / mid[:-1]))
    tol = float(np.float32(np.sqrt(mid[g] * mid[g + 1])))
    assert mid[g] * 1.0001 < tol < mid[g + 1] / 1.0001, "no gap wide enough around the chosen tolerance"
    # what the model says of the rectangle at that tolerance
    act2 = select_unconverged(*after[2], cnt(2), tol, 0.0) != 0
    act3 = act2 & (select_unconverged(*after[3], cnt(3), tol, 0.0) != 0)
    want_n = np.where(act3, spp, np.where(act2, sum(counts[:3]), sum(counts[:2])))
    assert (want_n == spp).any() and (want_n < spp).any()
    acc, _, st = gpu_ctx.render_adaptive(desc, tol, passes=P, min_passes=M)
    torch.cuda.synchronize()
    n = acc.n.cpu().numpy()
    assert np.array_equal(n[r0:r1, c0:c1], want_n)
    assert (n == spp).any() and (n < spp).any()
    assert all(a >= b for a, b in zip(st["active"], st["active"][1:])) and st["active"][-1] < W * H
    assert set(np.unique(n).tolist()) <= {sum(counts[:k]) for k in range(M, P + 1)}
    assert st["samples_total"] == int(n.sum()) < W * H * spp


# ---- 6. refusals ----
def test_refusals_leave_the_buffers_alone(dsrt, gpu_ctx):
    capi, lib = dsrt.capi, dsrt.lib
    hs, scene, W, H, spp, depth = parity_case(dsrt, "lights", SEED, 8)
    gpu_ctx.upload(scene)
    s0, sq0, n0 = _sentinels(W, H)
    s, sq, n = _dev64(s0), _dev64(sq0), _dev32(n0)
    mask0 = (np.arange(W * H, dtype=np.uint32) % 3 == 0).astype(np.uint8) * 9
    mask = torch.from_numpy(mask0).to(DEV)
    out8 = torch.zeros(W * H * 3, dtype=torch.uint8, device=DEV)
    var = torch.zeros(W * H * 3, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None          # noqa: E731
    acc_of = lambda a, b=None: capi.DsrtAccum(ptr(a), ptr(b))                   # noqa: E731
    good = _desc(dsrt, W, H, spp, depth)

    def masked(desc, first, count, stride, acc, m=mask, ctx=gpu_ctx):
        return lib.dsrt_render_accumulate_masked(ctx._h, C.byref(desc), first, count, stride, C.byref(acc), ptr(m), ptr(n), None, None)

    def select(desc, acc, nn=n, m=mask, tol=0.1):
        return lib.dsrt_select_unconverged(gpu_ctx._h, C.byref(desc), C.byref(acc), ptr(nn), tol, 0.0, 0, UINT32_MAX, ptr(m), None, None)

    def resolve(desc, acc, nn=n, rgb=out8, v=None):
        return lib.dsrt_resolve_accumulated_counts(gpu_ctx._h, C.byref(desc), C.byref(acc), ptr(nn), ptr(rgb), None, ptr(v), None)

    def adaptive(desc, passes, min_passes, acc, nn=n, tol=0.1, ctx=gpu_ctx):
        ad = capi.DsrtAdaptive(passes, min_passes, tol, 0.0)
        return lib.dsrt_render_adaptive(ctx._h, C.byref(desc), C.byref(ad), C.byref(acc), ptr(nn), ptr(out8), None, None, None, None)

    rng0 = dsrt.make_desc(W, H, spp, depth, seed=SEED, rng_mode=0)
    cases = [
        ("masked: rng_mode 0", masked(rng0, 0, spp, 1, acc_of(s, sq)), -1),
        ("masked: shards", masked(_desc(dsrt, W, H, spp, depth, shard_count=2), 0, spp, 1, acc_of(s, sq)), -1),
        ("masked: NULL mask", masked(good, 0, spp, 1, acc_of(s, sq), m=None), -1),
        ("masked: collect_counters", masked(_desc(dsrt, W, H, spp, depth, collect_counters=1), 0, spp, 1, acc_of(s, sq)), -1),
        ("masked: NULL sum", masked(good, 0, spp, 1, acc_of(None, sq)), -1),
        ("masked: count 0", masked(good, 0, 0, 1, acc_of(s, sq)), -1),
        ("masked: past spp", masked(good, 2, 3, 3, acc_of(s, sq)), -1),
        ("select: no sum_sq", select(good, acc_of(s)), -1),
        ("select: rng_mode 0", select(rng0, acc_of(s, sq)), -1),
        ("select: NULL n", select(good, acc_of(s, sq), nn=None), -1),
        ("select: NULL mask", select(good, acc_of(s, sq), m=None), -1),
        ("select: negative tolerance", select(good, acc_of(s, sq), tol=-0.5), -1),
        ("select: NaN tolerance", select(good, acc_of(s, sq), tol=float("nan")), -1),
        ("resolve: variance without sum_sq", resolve(good, acc_of(s), v=var), -1),
        ("resolve: no output", resolve(good, acc_of(s, sq), rgb=None), -1),
        ("resolve: NULL n", resolve(good, acc_of(s, sq), nn=None), -1),
        ("adaptive: passes 0", adaptive(good, 0, 0, acc_of(s, sq)), -1),
        ("adaptive: passes above spp", adaptive(good, spp + 1, 1, acc_of(s, sq)), -1),
        ("adaptive: passes above 64", adaptive(_desc(dsrt, W, H, 100, depth), 65, 1, acc_of(s, sq)), -1),
        ("adaptive: min_passes above passes", adaptive(good, 4, 5, acc_of(s, sq)), -1),
        ("adaptive: min_passes 0", adaptive(good, 4, 0, acc_of(s, sq)), -1),
        ("adaptive: no sum_sq", adaptive(good, 4, 2, acc_of(s)), -1),
        ("adaptive: NULL n", adaptive(good, 4, 2, acc_of(s, sq), nn=None), -1),
        ("adaptive: rng_mode 0", adaptive(rng0, 4, 2, acc_of(s, sq)), -1),
        ("adaptive: collect_counters", adaptive(_desc(dsrt, W, H, spp, depth, collect_counters=1), 4, 2, acc_of(s, sq)), -1),
    ]
    fresh = dsrt.Context(0)
    try:
        cases.append(("masked: no scene", masked(good, 0, spp, 1, acc_of(s, sq), ctx=fresh), -6))
        cases.append(("adaptive: no scene", adaptive(good, 4, 2, acc_of(s, sq), ctx=fresh), -6))
    finally:
        fresh.close()
    for what, rc, want in cases:
        assert rc == want, (what, rc)
    assert lib.dsrt_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(_u64(s, s0.shape), s0) and np.array_equal(_u64(sq, sq0.shape), sq0)
    assert np.array_equal(n.cpu().numpy().view(np.uint32).reshape(H, W), n0) and np.array_equal(mask.cpu().numpy(), mask0)
    assert not out8.any() and not var.any()
    with pytest.raises(dsrt.DsrtError, match="collect_counters"):
        gpu_ctx.render_accumulate_masked(_desc(dsrt, W, H, spp, depth, collect_counters=1), 0, spp, 1, s, sq, mask, n)
    # ... and the same call, allowed, is a launch: the sentinel moves where the mask is set
    gpu_ctx.render_accumulate_masked(good, 0, spp, 1, s, sq, mask, n)
    torch.cuda.synchronize()
    moved = n.cpu().numpy().view(np.uint32).reshape(H, W) != n0
    assert np.array_equal(moved.reshape(-1), mask0 != 0)


# ---- 7. the CLI ----
def _read_ppm(path):
    data = open(path, "rb").read()
    parts = data.split(b"\n", 3)
    w, h = map(int, parts[1].split())
    return np.frombuffer(parts[3], np.uint8).reshape(h, w, 3)


def _read_pfm(path):
    data = open(path, "rb").read()
    head, dims, scale, rest = data.split(b"\n", 3)
    w, h = map(int, dims.split())
    c = 3 if head == b"PF" else 1
    return np.frombuffer(rest, "<f4").reshape(h, w, c)[::-1].reshape(h, w, c)


def test_cli_adaptive(dsrt, gpu_ctx, tmp_path):
    exe = os.path.join(ROOT, "deep-space-ray-tracer_amd", "dsrt_render")
    obj = os.path.join(ASSETS, "station_3k.obj")
    poses_txt = os.path.join(GOLDEN, "rendezvous_1s_dt0_01s.txt")
    W, H, spp, tol, P, M, floor = 64, 48, 24, 0.08, 6, 2, 0.02
    cmd = [exe, "--obj", obj, "--input_txt", poses_txt, "--width", str(W), "--height", str(H), "--spp", str(spp), "--frame", "98", "--frames", "1", "--rng-mode", "1",
           "--output_dir", str(tmp_path), "--adaptive", str(tol), "--adaptive-passes", str(P), "--adaptive-min-passes", str(M), "--adaptive-floor", str(floor), "--variance"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    hs = dsrt.HostScene().add_obj(obj)
    hs.build_bvh()
    fr = dsrt.pose_to_frame(dsrt.read_pose_file(poses_txt)[98])
    gpu_ctx.upload(hs.view(dsrt.frame_camera(fr, 40.0, W, H, spp, 50), tuple(fr.sun_dir_model)))
    desc = dsrt.make_desc(W, H, spp, 50, gamma=2.0, seed=1337, rng_mode=1)
    acc, (rgb, _, var), st = gpu_ctx.render_adaptive(desc, tol, passes=P, min_passes=M, floor=floor, want_var=True)
    torch.cuda.synchronize()
    n = acc.n.cpu().numpy()
    assert rgb.any() and (n < spp).any() and (n == spp).any()
    assert np.array_equal(_read_ppm(tmp_path / "frame_0098.ppm"), rgb.cpu().numpy())
    assert np.array_equal(_read_pfm(tmp_path / "frame_0098_spp.pfm")[..., 0], n.astype(np.float32))
    assert np.array_equal(_read_pfm(tmp_path / "frame_0098_var.pfm").view(np.uint32), var.cpu().numpy().view(np.uint32))
    assert f"adaptive: {st['passes_run']} of {P} passes" in r.stdout
    for extra in (["--passes", "2"], ["--gbuffer"]):
        r = subprocess.run(cmd + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and "--adaptive does not combine" in r.stderr
