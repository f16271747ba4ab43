"""The scheduling pre-pass on the GPU against its CPU model (tests/_schedule_model.py): cost words, culls, tile order, sched words, probe and reorder, the batch
table and the lists of a masked launch, read back through dsrt_selftest_read_schedule or run on hand-made arrays through dsrt_selftest_tile_order / _tile_reorder /
_batch_table.  Everything is integers and compared exactly; where the kernels leave an order open (inside a bin, inside a key) the result must lie in the model's
legal set.  Healthy scenes only.  The hand-made arrays and the station views are tests/test_schedule_host.py's, which holds the model itself to the oracle."""
import numpy as np
import pytest

import _schedule_model as M
from conftest import load_world
from test_oracle import CASES, SUN
from test_schedule_host import STATION_VIEWS, batch_cases, order_cases, reorder_cases, root_box, station_view

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

NO_CULLING, NO_PROBE = 2, 8                       # include/dsrt.h, DSRT_TUNE_*


@pytest.fixture(scope="module")
def station(dsrt):
    return load_world(dsrt, "station_3k")


_frames = {}


def _frame_model(oracle, hs, key, cam, scene, W, H, tile=8, cullable=True):
    """(hits, culled blocks or None) of a view, computed once per module."""
    k = (key, W, H, tile)
    if k not in _frames:
        culled = None
        if cullable:
            lo, hi = root_box(hs)
            culled, decided = M.frame_culled_blocks(lo, hi, M.camera12(cam), W, H, tile)
            assert decided.all()                                       # (test_schedule_host.py asserts it for the named views on the CPU)
        _frames[k] = (M.centre_hits(oracle.lib, scene, W, H), culled)
    return _frames[k]


def _read_pre(ctx, mine, frame=0):
    """(cost words, sched[5], list_len[2], order[n_live]) of frame `frame` of the context's last launch."""
    base = frame * (mine + M.PRE_PAD)
    w = ctx.read_schedule("tile_cost", base, mine + M.LIST_LEN_AT + 2)
    sched = [int(v) for v in w[mine + M.SCHED_AT:mine + M.SCHED_AT + 5]]
    order = ctx.read_schedule("tile_order", base, sched[1]) if sched[1] else np.zeros(0, np.uint32)
    return w[:mine].copy(), sched, [int(v) for v in w[mine + M.LIST_LEN_AT:mine + M.LIST_LEN_AT + 2]], order


def _check_frame(ctx, st, want_cost, tile, rng_mode, spp, what):
    """The last single-frame launch's cost words are `want_cost`; its sched words are the model's for them and the lanes the launch had; its order is legal; its
    stats count the tiles the model drops.  -> (sched, order)."""
    mine = want_cost.size
    cost, sched, _, order = _read_pre(ctx, mine)
    assert np.array_equal(cost, want_cost), (what, np.nonzero(cost != want_cost)[0][:8], cost[cost != want_cost][:8], want_cost[cost != want_cost][:8])
    ipp = M.host_slices(spp, rng_mode)[0]
    bins, want_sched, legal = M.tile_order(want_cost, tile, ipp, st.waves_launched * 64, spp)
    assert sched == want_sched, (what, sched, want_sched)
    assert legal.why_not(order) is None, (what, legal.why_not(order))
    assert st.tiles_total == mine and st.tiles_culled == int((want_cost == 0).sum()), what
    return sched, order


# ---------------------------------------------------------------- a. the array kernels on hand-made arrays ----------------------------------------------------------------
def test_tile_order_kernel_on_hand_made_costs(gpu_ctx):
    """Every edge of the bin rule, n across the block's 1024 threads, every threshold of spread and slices (test_schedule_host.order_cases)."""
    for name, cost, tile, ipp, rl, spp in order_cases():
        order, sched = gpu_ctx.selftest_tile_order(cost, tile, ipp, rl, spp)
        bins, want, legal = M.tile_order(cost, tile, ipp, rl, spp)
        assert [int(v) for v in sched] == want, (name, list(sched), want)
        assert legal.why_not(order[:want[1]]) is None, (name, legal.why_not(order[:want[1]]))
        assert (order[want[1]:] == M.M32).all(), name                         # nothing is written behind the live tiles


def test_tile_reorder_kernel_on_hand_made_work(gpu_ctx):
    for name, work, order, sched in reorder_cases():
        out = gpu_ctx.selftest_tile_reorder(work, order, sched)
        assert M.reorder_why_not(work, order, sched, out) is None, (name, M.reorder_why_not(work, order, sched, out))
        if len(set(M.reorder_keys(work, order[:sched[0]]).tolist())) == sched[0]:          # distinct keys: one legal result
            assert np.array_equal(out, M.tile_reorder(work, order, sched)), name


def test_batch_table_kernel_on_hand_made_sched_words(gpu_ctx):
    for name, rows, tt, rng_mode, spp, light, base in batch_cases():
        sched = np.zeros((len(rows), 7), np.uint32)                               # (a stride that is not the five words themselves)
        sched[:, :5] = rows
        table, total = gpu_ctx.selftest_batch_table(sched, tt, rng_mode, spp, light, base)
        fields, want_total = M.batch_table(rows, tt, rng_mode, spp, light, base)
        assert total == want_total, name
        for at, want in M.batch_table_words(fields).items():
            assert np.array_equal(table[:, at], want), (name, at, table[:, at], want)
        assert np.array_equal(table[:, M.B_IMAGE_SLOT], np.tile(np.arange(len(rows), dtype=np.uint32), 2)), name
        assert not table[:, :15].any() and not table[:, 22:].any(), name           # the cameras and the padding are not the kernel's to write


# ---------------------------------------------------------------- b. costs and culls of real frames ----------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(STATION_VIEWS))
def test_costs_culls_order_and_sched_of_station_views(dsrt, gpu_ctx, oracle, station, name):
    """One 1-spp render per variant, then the pre-pass's words: plain, DSRT_TUNE_NO_CULLING, rng_mode 1 at 8 and 250 samples (slices, chunk_len), and every rank
    of three (local tile k is global tile 3 k + rank)."""
    cam, scene, W, H = station_view(dsrt, station, name)
    hits, culled = _frame_model(oracle, station, name, cam, scene, W, H)
    gpu_ctx.upload(scene)
    want = M.tile_costs(hits, W, H, 8, culled_blocks=culled)
    assert (want == 0).any() == STATION_VIEWS[name][4]
    _, _, st = gpu_ctx.render_to_host(dsrt.make_desc(W, H, 1, 12))
    sched, order = _check_frame(gpu_ctx, st, want, 8, 0, 1, (name, "plain"))
    _, _, st = gpu_ctx.render_to_host(dsrt.make_desc(W, H, 1, 12, tune=(0, 0, 0, NO_CULLING)))
    every = M.tile_costs(hits, W, H, 8)
    assert (every & M.LIVE).all()
    _check_frame(gpu_ctx, st, every, 8, 0, 1, (name, "no culling"))
    for spp in (8, 250):
        _, _, st = gpu_ctx.render_to_host(dsrt.make_desc(W, H, spp, 12, rng_mode=1))
        s1, _ = _check_frame(gpu_ctx, st, want, 8, 1, spp, (name, "rng_mode 1", spp))
        assert (s1[3] - 1) * s1[4] < spp <= s1[3] * s1[4]
    live = set()
    for rank in range(3):
        desc = dsrt.make_desc(W, H, 1, 12, tile_size=8, shard_rank=rank, shard_count=3)
        part = torch.zeros(dsrt.shard_layout(desc)["rgb8_bytes_padded"], dtype=torch.uint8, device="cuda")
        st = gpu_ctx.render(desc, part.data_ptr(), stream=torch.cuda.current_stream().cuda_stream, want_stats=True)
        mine = M.tiling(W, H, 8, rank, 3)["mine"]
        assert dsrt.shard_layout(desc)["tiles_this_shard"] == mine
        _, o = _check_frame(gpu_ctx, st, M.tile_costs(hits, W, H, 8, rank, 3, culled), 8, 0, 1, (name, "rank", rank))
        live |= {int(k) * 3 + rank for k in o}
    assert live == {int(k) for k in order}                                 # together the ranks' live sets are the whole frame's


@pytest.mark.parametrize("tile", [16, 32])
def test_costs_and_culls_on_tiles_of_several_blocks(dsrt, gpu_ctx, oracle, station, tile):
    """97 x 61 in 16- and 32-pixel tiles: blocks partly and wholly outside the image (tested like any other: they can keep a tile alive), and the bin rule's
    light tiles that see geometry."""
    cam, scene, W, H = station_view(dsrt, station, "far", size=(97, 61))
    hits, culled = _frame_model(oracle, station, "far", cam, scene, W, H, tile)
    gpu_ctx.upload(scene)
    want = M.tile_costs(hits, W, H, tile, culled_blocks=culled)
    assert (want == 0).any() and (want & 0x7FFFFFFF).any()
    for rng_mode, spp in ((0, 1), (1, 8)):
        _, _, st = gpu_ctx.render_to_host(dsrt.make_desc(W, H, spp, 12, tile_size=tile, rng_mode=rng_mode))
        _check_frame(gpu_ctx, st, want, tile, rng_mode, spp, (tile, rng_mode))
    _, _, st = gpu_ctx.render_to_host(dsrt.make_desc(W, H, 1, 12, tile_size=tile, tune=(0, 0, 0, NO_CULLING)))
    _check_frame(gpu_ctx, st, M.tile_costs(hits, W, H, tile), tile, 0, 1, (tile, "no culling"))


def test_costs_with_spheres_and_on_frames_of_one_tile(dsrt, gpu_ctx, oracle, station):
    """`mixed` has spheres: nothing is culled and the pixels that see a sphere count.  Then frames that are one tile: 8 x 8, and 5 x 3 (a tile mostly outside)."""
    hs = load_world(dsrt, "mixed")
    W, H = 96, 64
    cam = dsrt.camera_look_at(*CASES["mixed"][1][:3], W, H, 4, 10)
    scene = hs.view(cam, SUN)
    hits, _ = _frame_model(oracle, hs, "mixed", cam, scene, W, H, cullable=False)
    assert len(hs.arrays()["spheres"]) > 0
    no_spheres = hs.view(cam, SUN)
    no_spheres.num_spheres = 0
    assert (hits & ~M.centre_hits(oracle.lib, no_spheres, W, H)).any()          # some pixel sees a sphere and no triangle: the count needs the sphere loop
    gpu_ctx.upload(scene)
    _, _, st = gpu_ctx.render_to_host(dsrt.make_desc(W, H, 1, 10))
    want = M.tile_costs(hits, W, H, 8)
    _check_frame(gpu_ctx, st, want, 8, 0, 1, "mixed")
    assert st.tiles_culled == 0 and (want == M.LIVE).any()                     # tiles that see nothing stay in the order
    for W, H in ((8, 8), (5, 3)):
        cam = dsrt.camera_look_at((25.0, 18.0, 70.0), (0.0, 0.0, 0.0), 40.0, W, H, 1, 12)
        scene = station.view(cam, SUN)
        hits, culled = _frame_model(oracle, station, "one tile", cam, scene, W, H)
        gpu_ctx.upload(scene)
        want = M.tile_costs(hits, W, H, 8, culled_blocks=culled)
        assert want.size == 1 and 0 < (int(want[0]) & 0x7FFFFFFF) <= W * H
        for rng_mode, spp in ((0, 1), (1, 8)):
            _, _, st = gpu_ctx.render_to_host(dsrt.make_desc(W, H, spp, 12, rng_mode=rng_mode))
            _check_frame(gpu_ctx, st, want, 8, rng_mode, spp, (W, H, rng_mode))


# ---------------------------------------------------------------- c. probe and reorder ----------------------------------------------------------------
@pytest.mark.parametrize("scale,tile,dealt", [(1.0, 8, True), (0.2, 16, False)])
def test_probe_work_and_the_reordered_heavy_tiles(dsrt, gpu_ctx, oracle, station, scale, tile, dealt):
    """The 96 x 54 frame of test_scheduling_switches_never_change_a_pixel at 256 spp, rng_mode 0: the probe runs.
    DEALT: at 8-pixel tiles 54 of the 84 tiles are heavy, 3456 heavy pixels for the 5376 lanes the launch has, so sched[2] < 64 and the heavy tiles are dealt
    costliest, cheapest, ...  SORTED: with the camera at a fifth of the distance and 16-pixel tiles every one of the 24 tiles is heavy, 6144 heavy pixels for
    6144 lanes, sched[2] == 64 and the heavy tiles are sorted.  (Which is which is asserted from the model below.)
    Work of a heavy tile: the probe renders PROBE_SPP = 4 samples of every pixel of the heavy tiles; every sample launches its camera ray before anything can end it
    (path_machine.h: ST_GEN sets `launch`, the ray start counts it, 8 bits saturating at 255), and a tile's word is the maximum over its pixels, of which a heavy
    tile has at least one inside the image: 4 <= work <= 255.  Tiles outside the heavy part are not probed: 0."""
    W, H, spp, depth = 96, 54, 256, CASES["station_near"][1][5]
    cam = dsrt.camera_look_at((12.0 * scale, 9.0 * scale, 38.0 * scale), (0.0, 0.0, 0.0), 40.0, W, H, spp, depth)
    scene = station.view(cam, SUN)
    hits, culled = _frame_model(oracle, station, ("near", scale), cam, scene, W, H, tile)
    gpu_ctx.upload(scene)
    want = M.tile_costs(hits, W, H, tile, culled_blocks=culled)
    mine = want.size
    # without the probe: a legal coverage order
    _, _, st = gpu_ctx.render_to_host(dsrt.make_desc(W, H, spp, depth, tile_size=tile, tune=(0, 0, 0, NO_PROBE)))
    sched, _ = _check_frame(gpu_ctx, st, want, tile, 0, spp, "no probe")
    assert (sched[2] < 64) == dealt, sched
    # with it
    _, _, st = gpu_ctx.render_to_host(dsrt.make_desc(W, H, spp, depth, tile_size=tile))
    cost, sched2, _, order = _read_pre(gpu_ctx, mine)
    bins, want_sched, legal = M.tile_order(want, tile, 1, st.waves_launched * 64, spp)
    assert np.array_equal(cost, want) and sched2 == want_sched == sched
    n_heavy = sched[0]
    heavy_set, light_set = np.nonzero((bins >= 0) & (bins < 64))[0], np.nonzero(bins == 64)[0]
    assert n_heavy == heavy_set.size >= 3
    work = gpu_ctx.read_schedule("tile_work", 0, mine)
    is_heavy = np.zeros(mine, bool)
    is_heavy[heavy_set] = True
    assert not work[~is_heavy].any()
    assert (work[is_heavy] >= M.PROBE_SPP).all() and (work[is_heavy] <= 255).all(), work[is_heavy]
    assert len(set(work[is_heavy].tolist())) > 1                               # (the probe tells tiles apart, or this test would not see the sort)
    assert sorted(order[n_heavy:].tolist()) == light_set.tolist()               # the light part: still the coverage order's, any order inside the one bin
    why = M.reorder_why_not(work, np.concatenate([heavy_set, order[n_heavy:]]), sched, order)
    assert why is None, why


# ---------------------------------------------------------------- d. batch ----------------------------------------------------------------
@pytest.mark.parametrize("rng_mode,spp", [(1, 8), (0, 256)])
def test_batch_prepass_words_and_table(dsrt, gpu_ctx, oracle, station, rng_mode, spp):
    """Three cameras in one launch: near, LOOKING AWAY (no live tile, between two frames that have some), far.  Every frame's cost, sched and order words
    pre_stride apart, and both table entries per frame, equal the model; every image is the single-frame render's.  At 256 spp in rng_mode 0 every frame is probed
    (tile_work holds the last frame's)."""
    W, H, depth = 64, 40, 12
    views = [("near", (12.0, 9.0, 38.0), (0.0, 0.0, 0.0)), ("away", (0.0, 0.0, 300.0), (0.0, 0.0, 600.0)), ("far", (-0.7, 0.0, 260.0), (0.0, 0.0, 0.0))]
    cams = [dsrt.camera_look_at(a, b, 40.0, W, H, spp, depth) for _, a, b in views]
    gpu_ctx.upload(station.view(cams[0], SUN))
    n = len(cams)
    rgb = torch.zeros(n * H * W * 3, dtype=torch.uint8, device="cuda")
    st = gpu_ctx.render_batch(dsrt.make_desc(W, H, spp, depth, rng_mode=rng_mode), cams, [SUN] * n, rgb.data_ptr(), stream=torch.cuda.current_stream().cuda_stream,
                              want_stats=True)
    assert st.device_flags == 0
    mine = M.tiling(W, H)["mine"]
    ipp, _, light = M.host_slices(spp, rng_mode)
    rows, lives = [], []
    for f, (name, _, _) in enumerate(views):
        hits, culled = _frame_model(oracle, station, ("batch", name), cams[f], station.view(cams[f], SUN), W, H)
        want = M.tile_costs(hits, W, H, 8, culled_blocks=culled)
        cost, sched, _, order = _read_pre(gpu_ctx, mine, f)
        assert np.array_equal(cost, want), (name, cost, want)
        bins, want_sched, legal = M.tile_order(want, 8, ipp, 0, spp)               # resident_lanes = 0: the batch's own setting
        assert sched == want_sched, (name, sched, want_sched)
        if rng_mode == 1:
            assert legal.why_not(order) is None, (name, legal.why_not(order))
        else:                                                                        # probed: the heavy part re-sorted (sched[2] == 64), the light part as it was
            heavy_set = np.nonzero((bins >= 0) & (bins < 64))[0]
            assert sorted(order[:sched[0]].tolist()) == heavy_set.tolist() and sorted(order[sched[0]:].tolist()) == np.nonzero(bins == 64)[0].tolist(), name
            if f == n - 1:
                work = gpu_ctx.read_schedule("tile_work", 0, mine)
                assert sched[0] >= 2 and (work[heavy_set] >= M.PROBE_SPP).all() and not np.delete(work, heavy_set).any()
                why = M.reorder_why_not(work, np.concatenate([heavy_set, order[sched[0]:]]), sched, order)
                assert why is None, why
        rows.append(sched)
        lives.append(sched[1])
    assert lives[1] == 0 and lives[0] > 0 and lives[2] > 0
    table = gpu_ctx.read_schedule("batch_table", 0, 2 * n * M.BATCH_WORDS).reshape(2 * n, M.BATCH_WORDS)
    fields, total = M.batch_table(rows, 64, rng_mode, spp, light, [f * (mine + M.PRE_PAD) for f in range(n)])
    for at, want in M.batch_table_words(fields).items():
        assert np.array_equal(table[:, at], want), (at, table[:, at], want)
    assert int(table[-1, M.B_ITEM_END]) == total
    assert np.array_equal(table[:, M.B_IMAGE_SLOT], np.tile(np.arange(n, dtype=np.uint32), 2))
    for f in range(n):
        for e in (f, n + f):
            assert np.array_equal(table[e, :12], M.camera12(cams[f]).view(np.uint32)) and np.array_equal(table[e, 12:15], np.float32(SUN).view(np.uint32))
    got = rgb.cpu().numpy().reshape(n, H, W, 3)
    for f in range(n):
        gpu_ctx.set_camera_sun(cams[f], SUN)
        alone, _, _ = gpu_ctx.render_to_host(dsrt.make_desc(W, H, spp, depth, rng_mode=rng_mode))
        assert np.array_equal(got[f], alone), views[f][0]
    assert got[0].any() and not got[1].any()


# ---------------------------------------------------------------- e. lists ----------------------------------------------------------------
@pytest.mark.parametrize("tile", [8, 16, 32])
def test_pixel_lists_of_masked_launches(dsrt, gpu_ctx, station, tile):
    """dsrt_render_accumulate_masked on 97 x 61: the two lists, the per-block offsets and the two lengths are the model's for the order that was read back --
    order position, then block, then lane."""
    W, H, spp = 97, 61, 8
    cam = dsrt.camera_look_at((12.0, 9.0, 38.0), (0.0, 0.0, 0.0), 40.0, W, H, spp, 12)
    gpu_ctx.upload(station.view(cam, SUN))
    desc = dsrt.make_desc(W, H, spp, 12, rng_mode=1, tile_size=tile)
    t = M.tiling(W, H, tile)
    mine, tt, bpt = t["mine"], tile * tile, (tile // 8) ** 2
    edge = np.zeros((H, W), np.uint8)
    edge[:, W - 1] = 1
    edge[H - 1, :] = 1
    masks = (("Bernoulli(0.3)", (np.random.default_rng(11).random((H, W)) < 0.3).astype(np.uint8)), ("last row and column", edge),
             ("all ones", np.ones((H, W), np.uint8)), ("empty", np.zeros((H, W), np.uint8)))
    sums = torch.zeros(W * H * 3, dtype=torch.int64, device="cuda")
    for what, mask in masks:
        gpu_ctx.render_accumulate_masked(desc, 0, 4, 2, sums, None, torch.from_numpy(mask.reshape(-1)).to("cuda"), None, want_stats=True)
        cost, sched, list_len, order = _read_pre(gpu_ctx, mine)
        assert 0 < sched[0] < sched[1] <= mine and M.LegalOrders([M.tile_bin(int(c), tile) for c in cost]).why_not(order) is None
        words, lh, ll, offs = M.pixel_lists(order, sched, mask, W, H, tile)
        assert list_len == [lh, ll], (what, list_len, lh, ll)
        got = gpu_ctx.read_schedule("pixel_list", 0, mine * tt + sched[1] * bpt)
        assert np.array_equal(got[:lh], words[:lh]), what
        at = sched[0] * tt
        assert np.array_equal(got[at:at + ll], words[at:at + ll]), what
        assert np.array_equal(got[mine * tt:], offs), what
        if what == "all ones":                                                       # every pixel of every live tile exactly once
            both = np.concatenate([got[:lh], got[at:at + ll]]).astype(np.int64)
            seen = np.zeros((H, W), np.int64)
            np.add.at(seen, (both >> 16, both & 0xFFFF), 1)
            live = np.zeros((H, W), np.int64)
            for k in order:
                live[(int(k) // t["tiles_x"]) * tile:(int(k) // t["tiles_x"] + 1) * tile, (int(k) % t["tiles_x"]) * tile:(int(k) % t["tiles_x"] + 1) * tile] = 1
            assert np.array_equal(seen, live) and lh + ll == int(live.sum())


# ---------------------------------------------------------------- f. what the hooks refuse ----------------------------------------------------------------
def test_schedule_hooks_refuse_what_they_cannot_do(dsrt, gpu_ctx, station):
    lib = dsrt.lib
    sentinel = np.full(16, 0xA5A5A5A5, np.uint32)
    out = sentinel.copy()
    ctx = dsrt.Context(0)
    try:
        for array in range(5):                                                      # before any launch: no array exists
            assert lib.dsrt_selftest_read_schedule(ctx._h, array, 0, 1, out.ctypes.data) == -1
        W, H = 40, 24
        cam = dsrt.camera_look_at((12.0, 9.0, 38.0), (0.0, 0.0, 0.0), 40.0, W, H, 1, 12)
        ctx.upload(station.view(cam, SUN))
        ctx.render_to_host(dsrt.make_desc(W, H, 1, 12))
        words = M.tiling(W, H)["mine"] + M.PRE_PAD                                  # this context's first launch: the buffers are exactly this long
        for array in ("tile_cost", "tile_order", "tile_work"):
            assert ctx.read_schedule(array, 0, words).size == words and ctx.read_schedule(array, words - 1, 1).size == 1
            for first, count in ((0, words + 1), (words, 1), (1, words), (1 << 40, 1), (0, 1 << 62), (2, (1 << 64) - 1), (0, 0)):
                assert lib.dsrt_selftest_read_schedule(ctx._h, ctx.SCHEDULE_ARRAYS.index(array), first, count, out.ctypes.data) == -1, (array, first, count)
        for array in (3, 4, 5, -1, 1 << 20):                                        # no batch and no masked launch yet; arrays that do not exist
            assert lib.dsrt_selftest_read_schedule(ctx._h, array, 0, 1, out.ctypes.data) == -1, array
        assert lib.dsrt_selftest_read_schedule(ctx._h, 0, 0, 1, None) == -1 and lib.dsrt_selftest_read_schedule(None, 0, 0, 1, out.ctypes.data) == -1
        assert b"dsrt_selftest_read_schedule" in lib.dsrt_last_error()
    finally:
        ctx.close()
    cost = np.array([64 | M.LIVE, 65 | M.LIVE], np.uint32)                          # the runners: what would take a kernel outside its arrays
    sched5, order = out[:5], out[5:7]
    h = gpu_ctx._h
    assert lib.dsrt_selftest_tile_order(h, cost.ctypes.data, 2, 8, 1, 0, 8, order.ctypes.data, sched5.ctypes.data) == -1              # more pixels than a tile has
    for tile, ipp, spp, n in ((12, 1, 8, 2), (0, 1, 8, 2), (2048, 1, 8, 2), (8, 0, 8, 2), (8, 1, 0, 2), (8, 1, 8, -1)):
        assert lib.dsrt_selftest_tile_order(h, cost[:1].ctypes.data, min(n, 1), tile, ipp, 0, spp, order.ctypes.data, sched5.ctypes.data) == -1, (tile, ipp, spp, n)
    assert lib.dsrt_selftest_tile_order(h, None, 1, 8, 1, 0, 8, order.ctypes.data, sched5.ctypes.data) == -1
    assert lib.dsrt_selftest_tile_order(h, cost.ctypes.data, 1, 8, 1, 0, 8, order.ctypes.data, None) == -1
    work, ord3 = np.array([1, 2, 3], np.uint32), np.array([0, 1, 3], np.uint32)
    keep = ord3.copy()
    for s0, n_order in ((3, 3), (4, 3), (2, 1)):                                    # an entry beyond the work array; more heavy entries than entries
        s = np.array([s0, 3, 64, 1, 8], np.uint32)
        assert lib.dsrt_selftest_tile_reorder(h, work.ctypes.data, 3, ord3.ctypes.data, n_order, s.ctypes.data) == -1, (s0, n_order)
    assert lib.dsrt_selftest_tile_reorder(h, work.ctypes.data, 3, ord3.ctypes.data, 3, None) == -1
    rows = np.array([[2, 1, 64, 1, 8]], np.uint32)                                  # more heavy tiles than live ones
    base, table, total = np.zeros(1, np.uint32), out[:1], out[7:8]
    assert lib.dsrt_selftest_batch_table(h, rows.ctypes.data, 5, 1, 64, 0, 8, 8, base.ctypes.data, table.ctypes.data, total.ctypes.data) == -1
    rows[0, 0] = 1
    for stride, frames, rng_mode, spp, light in ((4, 1, 0, 8, 8), (5, 0, 0, 8, 8), (5, 1, 2, 8, 8), (5, 1, 0, 0, 8), (5, 1, 1, 8, 0)):
        assert lib.dsrt_selftest_batch_table(h, rows.ctypes.data, stride, frames, 64, rng_mode, spp, light, base.ctypes.data, table.ctypes.data, total.ctypes.data) == -1
    assert lib.dsrt_selftest_batch_table(h, rows.ctypes.data, 5, 1, 64, 0, 8, 8, base.ctypes.data, None, total.ctypes.data) == -1
    assert np.array_equal(out, sentinel) and np.array_equal(ord3, keep)             # every refusal left its outputs alone
