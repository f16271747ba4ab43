"""The CPU model of the scheduling pre-pass (tests/_schedule_model.py) held to things that do not go through it: hand-computed answers, brute-force restatements,
the oracle's renders, and the properties DESIGN.md section 4 promises.  No GPU.  tests/test_gpu_schedule.py feeds the same hand-made arrays (the *_CASES functions
below) and the same views through the kernels."""
import ctypes as C
import itertools

import numpy as np
import pytest

import _schedule_model as M
from conftest import load_world
from test_oracle import SUN

# station_3k as tests/test_gpu_parity.py::test_empty_tile_culling_is_exact looks at it: (lookfrom, lookat, W, H, culls something)
STATION_VIEWS = {
    "far": ((-0.7, 0.0, 260.0), (0.0, 0.0, 0.0), 200, 112, True),
    "ragged": ((60.0, 45.0, 120.0), (30.0, 10.0, 0.0), 157, 83, True),
    "edge": ((0.0, 0.0, 300.0), (250.0, 0.0, 0.0), 96, 64, True),
    "inside": ((0.5, 0.2, 0.3), (10.0, 0.0, 0.0), 96, 64, False),
}


def station_view(dsrt, hs, name, spp=8, depth=12, size=None):
    lookfrom, lookat, W, H, _ = STATION_VIEWS[name]
    if size:
        W, H = size
    cam = dsrt.camera_look_at(lookfrom, lookat, 40.0, W, H, spp, depth)
    return cam, hs.view(cam, SUN), W, H


def root_box(hs):
    root = hs.arrays()["nodes"][0]                     # scene_pack.hip: the root box is node 0's
    return root["bbox_min"], root["bbox_max"]


# ---------------------------------------------------------------- hand-made arrays, shared with the GPU tests ----------------------------------------------------------------
def edge_costs(tile):
    """Cost words at every edge of the bin rule, with and without bit 31: 0, 1, full/64 - 1, full/64, full - 1, full pixels."""
    full = tile * tile
    counts = sorted({0, 1, max(0, full // 64 - 1), full // 64, full - 1, full})
    return [c | live for c in counts for live in (0, M.LIVE)]


def order_cases():
    """(name, cost, tile, items_per_pixel, resident_lanes, spp) for dsrt_tile_order_kernel."""
    rng = np.random.default_rng(5)
    out = []
    for tile in (8, 16, 32):
        full = tile * tile
        e = np.array(edge_costs(tile), np.uint32)
        out.append((f"edges tile {tile}", e, tile, 1, 4096, 8))
        out.append((f"edges tile {tile}, rng_mode 1", e[::-1].copy(), tile, 8, 4096, 64))
        for n in (0, 1, 2, 1023, 1024, 1025):
            cost = rng.choice(np.concatenate([e, rng.integers(0, full + 1, 24).astype(np.uint32) | np.uint32(M.LIVE)]), n).astype(np.uint32)
            out.append((f"n {n} tile {tile}", cost, tile, 1 if n % 2 else 8, 65536, 250))
    for name, word in (("all full", 64 | M.LIVE), ("all light", M.LIVE), ("all dead", 0), ("all one pixel", 1 | M.LIVE)):
        out.append((name, np.full(1500, word, np.uint32), 8, 8, 1 << 18, 64))
        out.append((name + ", no lanes", np.full(9, word, np.uint32), 8, 1 if word & 1 else 8, 0, 250))      # a batch frame: with no heavy tile, heavy_items == lanes == 0
    # the spread threshold: resident_lanes at, one below and one above heavy_items (items_per_pixel 1: heavy_items = n_heavy * tile^2 whatever the lanes) ...
    cost = np.array([64 | M.LIVE] * 37 + [M.LIVE] * 11 + [0] * 5 + [9 | M.LIVE] * 3, np.uint32)
    heavy_items = 40 * 64
    for rl in (heavy_items - 1, heavy_items, heavy_items + 1, 3 * heavy_items + 1, 64 * heavy_items, 64 * heavy_items + 1, 1 << 20, 0):
        out.append((f"spread, lanes {rl}", cost, 8, 1, rl, 1000))
    # ... and the slice doubling of rng_mode 1: heavy_pixels * slices * 2 <= resident_lanes at 8 -> 16, 16 -> 32, 32 -> 64, each at, below and above
    for slices in (8, 16, 32):
        for d in (-1, 0, 1):
            out.append((f"slices {slices} -> {2 * slices}, lanes {d:+d}", cost, 8, 8, heavy_items * slices * 2 + d, 1000))
    # samples that do not divide, both kinds of launch, and the batch's resident_lanes = 0
    for spp, ipp, rl in itertools.product((1, 7, 8, 9, 63, 64, 250, 1000), (1, 8), (0, 1 << 20)):
        out.append((f"spp {spp} ipp {ipp} lanes {rl}", cost, 8, ipp, rl, spp))
    return out


def reorder_cases():
    """(name, work, order, sched) for dsrt_tile_reorder_kernel: sched[0] heavy entries, sched[2] < 64 = dealt."""
    rng = np.random.default_rng(6)
    out = []
    for n_heavy in (0, 1, 2, 3, 4, 5):
        order = rng.permutation(9).astype(np.uint32)                     # 9 tiles in the order, the first n_heavy of them heavy
        for spread in (63, 64, 1):
            for name, work in (("distinct", rng.permutation(9) * 20 + 5), ("equal", np.full(9, 17)), ("dominant", np.where(np.arange(9) == order[0], 255, 3)), ("zero", np.zeros(9))):
                out.append((f"n_heavy {n_heavy} spread {spread} work {name}", work.astype(np.uint32), order, [n_heavy, 9, spread, 1, 256]))
    for n in (1023, 1024, 1025, 2500):                                       # more heavy tiles than the block has threads
        order = rng.permutation(n + 40).astype(np.uint32)
        work = rng.integers(0, 256, n + 40).astype(np.uint32)
        for spread in (12, 64):
            out.append((f"n_heavy {n} spread {spread}", work, order, [n, n + 40, spread, 1, 256]))
    return out


def batch_cases():
    """(name, sched rows, tt, rng_mode, spp, light_chunk_len, order_base) for dsrt_batch_table_kernel."""
    heavy = (0, 1, 7, 8, 9, 17)
    rows = [[h, h + 5, 64, 8, 32] for h in heavy]
    base = [i * 300 for i in range(len(heavy))]
    gap = [[12, 20, 64, 16, 16], [0, 0, 64, 64, 4], [3, 3, 64, 8, 32]]        # a frame with no live tile between two live ones
    big = [[100000, 100001, 64, 64, 16]] * 3                                    # 6.5e9 items per frame: the total saturates
    out = []
    for rng_mode, spp, light in ((0, 256, 256), (1, 250, 128), (1, 8, 128)):
        out.append((f"heavy counts, rng_mode {rng_mode} spp {spp}", rows, 64, rng_mode, spp, light, base))
        out.append((f"empty frame, rng_mode {rng_mode} spp {spp}", gap, 256, rng_mode, spp, light, [0, 1000, 2000]))
    out.append(("saturates", big, 1024, 1, 1000, 128, [0, 200000, 400000]))
    return out


# ---------------------------------------------------------------- cull geometry and hit counts against the oracle ----------------------------------------------------------------
@pytest.fixture(scope="module")
def station(dsrt):
    return load_world(dsrt, "station_3k")


@pytest.mark.parametrize("name", sorted(STATION_VIEWS))
def test_cull_model_is_decided_and_every_culled_block_is_black_in_the_oracle(dsrt, oracle, station, name):
    cam, scene, W, H = station_view(dsrt, station, name)
    lo, hi = root_box(station)
    culled, decided = M.frame_culled_blocks(lo, hi, M.camera12(cam), W, H)
    assert decided.all(), f"{(~decided).sum()} undecided blocks"                      # the condition the GPU comparison rests on: none in these views
    assert culled.any() == STATION_VIEWS[name][4]
    rgb, f32, _ = oracle.render(scene, W, H)
    assert rgb.any() or name == "edge"                 # (the station lies just outside that frame: its footprint reaches blocks that no sample hits)
    for br, bc in zip(*np.nonzero(culled)):
        assert not rgb[br * 8:br * 8 + 8, bc * 8:bc * 8 + 8].any() and not f32[br * 8:br * 8 + 8, bc * 8:bc * 8 + 8].any(), (br, bc)
    # and no culled block holds a pixel whose centre ray hits: the cost words of a culled and an unculled pre-pass count the same pixels
    hits = M.centre_hits(oracle.lib, scene, W, H)
    assert hits.any() == rgb.any()
    a, b = M.tile_costs(hits, W, H, 8, culled_blocks=culled), M.tile_costs(hits, W, H, 8)
    assert np.array_equal(a & 0x7FFFFFFF, b & 0x7FFFFFFF) and int((a & 0x7FFFFFFF).sum()) == int(hits.sum())
    assert np.array_equal(a == 0, culled.reshape(-1)) and (b & M.LIVE).all()


def test_cull_model_on_larger_tiles_tests_the_blocks_beyond_the_image(dsrt, station):
    cam, scene, W, H = station_view(dsrt, station, "far", size=(97, 61))
    lo, hi = root_box(station)
    c8, d8 = M.frame_culled_blocks(lo, hi, M.camera12(cam), W, H, 8)
    for tile in (16, 32):
        c, d = M.frame_culled_blocks(lo, hi, M.camera12(cam), W, H, tile)
        assert d.all() and c.shape == (-(-H // tile) * tile // 8, -(-W // tile) * tile // 8)
        assert np.array_equal(c[:c8.shape[0], :c8.shape[1]], c8)                      # a block's verdict does not depend on the tiling
    assert d8.all() and c8.any() and not c8.all()


def test_hit_counts_equal_the_oracles_primary_hits_where_one_counter_covers_them(dsrt, oracle, station):
    """primary_hits counts JITTERED samples, the pre-pass centre rays; the two are the same number only where every ray of the frame agrees: a view away from the
    station (no sample hits, no centre ray hits) and a triangle that fills the frame (every sample hits, every centre ray hits)."""
    W, H = 40, 24
    cam = dsrt.camera_look_at((0.0, 0.0, 300.0), (0.0, 0.0, 600.0), 40.0, W, H, 4, 4)
    scene = station.view(cam, SUN)
    _, _, cnt = oracle.render(scene, W, H)
    hits = M.centre_hits(oracle.lib, scene, W, H)
    assert cnt["samples"] == W * H * 4 and cnt["primary_hits"] == 0 and int(hits.sum()) == 0
    assert not M.tile_costs(hits, W, H, 8).astype(np.int64).__and__(0x7FFFFFFF).any()
    tri = np.zeros(1, dsrt.capi.TRI_DTYPE)
    tri["v"][0] = [(-100.0, -100.0, -1.0), (100.0, -100.0, -1.0), (0.0, 150.0, 1.0)]      # (tilted: the slab test never enters a root box of no thickness)
    tri["n"][0] = [(0, 0, 1)] * 3
    tri["albedo_tex"] = -1
    mats = np.zeros(1, dsrt.capi.MAT_DTYPE)
    mats["albedo"], mats["albedo_tex"] = 0.5, -1
    hs = dsrt.HostScene().add_arrays(tris=tri, mats=mats)
    hs.build_bvh()
    cam = dsrt.camera_look_at((0.0, 0.0, 10.0), (0.0, 0.0, 0.0), 40.0, W, H, 4, 4)
    scene = hs.view(cam, SUN)
    _, _, cnt = oracle.render(scene, W, H)
    hits = M.centre_hits(oracle.lib, scene, W, H)
    assert cnt["primary_hits"] == cnt["samples"] == W * H * 4 and hits.all()
    cost = M.tile_costs(hits, W, H, 16)
    assert int((cost & 0x7FFFFFFF).sum()) * 4 == cnt["primary_hits"] and (cost & M.LIVE).all()
    assert [int(c) & 0x7FFFFFFF for c in cost] == [256, 256, 128, 128, 128, 64]      # 40 x 24 in 16-pixel tiles: 16 + 16 + 8 columns, 16 + 8 rows


def test_tile_costs_shards_deal_the_global_tiles_round_robin():
    W, H, tile = 61, 45, 8
    hits = np.random.default_rng(2).random((H, W)) < 0.4
    culled = np.random.default_rng(3).random((6, 8)) < 0.3
    whole = M.tile_costs(hits, W, H, tile, culled_blocks=culled)
    assert whole.size == 48 and np.array_equal(whole == 0, culled.reshape(-1))
    for k, (ty, tx) in enumerate(itertools.product(range(6), range(8))):
        if not culled[ty, tx]:
            assert int(whole[k]) == M.LIVE + int(hits[ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8].sum())
    seen = np.zeros(48, bool)
    for rank in range(3):
        part = M.tile_costs(hits, W, H, tile, rank, 3, culled)
        assert np.array_equal(part, whole[rank::3])
        seen[rank::3] = True
    assert seen.all()


# ---------------------------------------------------------------- order and sched ----------------------------------------------------------------
def test_bin_rule_known_answers():
    assert [M.tile_bin(c, 8) for c in (0, M.LIVE, 1, 1 | M.LIVE, 63 | M.LIVE, 64 | M.LIVE, 32)] == [-1, 64, 63, 63, 1, 0, 32]
    # 16- and 32-pixel tiles: fewer than tile^2 / 64 pixels is bin 64, a LIGHT tile although it sees geometry
    assert [M.tile_bin(c | M.LIVE, 16) for c in (0, 3, 4, 7, 8, 255, 256)] == [64, 64, 63, 63, 62, 1, 0]
    assert [M.tile_bin(c | M.LIVE, 32) for c in (0, 15, 16, 1023, 1024)] == [64, 64, 63, 1, 0]
    bins, sched, legal = M.tile_order(np.array([3 | M.LIVE, 4 | M.LIVE, 0, M.LIVE], np.uint32), 16, 1, 0, 8)
    assert sched[:2] == [1, 3] and list(legal.one()) == [1, 0, 3]


def test_sched_known_answers():
    cost = np.array([64 | M.LIVE] * 37 + [M.LIVE] * 11 + [0] * 5 + [9 | M.LIVE] * 3, np.uint32)       # 40 heavy tiles of 51 live
    s = lambda ipp, rl, spp: M.tile_order(cost, 8, ipp, rl, spp)[1]
    assert s(1, 2559, 1000) == [40, 51, 64, 1, 1000] and s(1, 2560, 1000) == [40, 51, 64, 1, 1000]
    assert s(1, 2561, 1000) == [40, 51, 64, 1, 1000]                 # ceil(2560 * 64 / 2561) = 64
    assert s(1, 7681, 1000) == [40, 51, 22, 1, 1000]                 # ceil(163840 / 7681) = 22
    assert s(1, 163840, 1000)[2] == 1 and s(1, 163841, 1000)[2] == 1 and s(1, 1 << 30, 1000)[2] == 1
    assert s(8, 40959, 1000) == [40, 51, 33, 8, 125]                 # 2560 pixels x 8 x 2 = 40960 > lanes: 8 slices; 20480 items: ceil(1310720 / 40959) = 33
    assert s(8, 40960, 1000) == [40, 51, 64, 16, 63]                 # 16 slices of ceil(1000 / 16) = 63; 40960 items = the lanes: no spread
    assert s(8, 1 << 20, 1000) == [40, 51, 10, 63, 16]               # 64 slices -> chunk 16 -> ceil(1000 / 16) = 63 slices
    assert s(8, 0, 250) == [40, 51, 64, 8, 32] and s(8, 0, 8) == [40, 51, 64, 8, 1] and s(8, 0, 7) == [40, 51, 64, 7, 1]
    assert s(8, 1 << 20, 9) == [40, 51, 1, 5, 2]                     # 8 slices (16 > 9) -> chunk 2 -> 5 slices; 12800 items: ceil(819200 / 1048576) = 1
    assert s(8, 0, 1) == [40, 51, 64, 1, 1]
    assert M.tile_order(np.zeros(7, np.uint32), 8, 8, 0, 1000)[1] == [0, 0, 64, 63, 16]       # no heavy pixel: the doubling's second condition is 0 <= lanes


@pytest.mark.parametrize("case", order_cases(), ids=lambda c: c[0])
def test_order_model_properties(case):
    _, cost, tile, ipp, rl, spp = case
    bins, sched, legal = M.tile_order(cost, tile, ipp, rl, spp)
    full = tile * tile
    pixels = cost.astype(np.int64) & 0x7FFFFFFF
    live = cost != 0
    # brute force, in the bin rule's own words: a live tile is heavy iff at least 1/64 of its pixels see geometry
    assert sched[1] == int(live.sum()) and sched[0] == int((live & (pixels * 64 >= full)).sum())
    n_heavy, n_live, spread, slices, chunk_len = sched
    assert 1 <= spread <= 64 and slices >= 1 and chunk_len >= 1
    assert (slices - 1) * chunk_len < spp <= slices * chunk_len                                   # the slices cover the samples, none is empty
    if ipp == 1:
        assert (slices, chunk_len) == (1, spp)
    else:
        assert slices <= max(ipp, 64) and (slices <= ipp or n_heavy * full * slices <= max(rl, 0) or n_heavy == 0)
    items = n_heavy * full * slices
    if items >= rl:
        assert spread == 64
    else:
        assert spread == max(1, -(-items * 64 // rl))
    one = legal.one()
    assert one in legal and len(one) == n_live
    if n_live:
        key = np.minimum(64, pixels[one] * 64 // full)
        assert (np.diff(key) <= 0).all()                                                           # costliest first
        assert (pixels[one[:n_heavy]] * 64 >= full).all() and (pixels[one[n_heavy:]] * 64 < full).all()
    if n_live >= 2:
        assert np.concatenate([one[:-1], one[:1]]) not in legal                                    # a tile twice
        assert one[:-1] not in legal and np.concatenate([one, one[:1]]) not in legal
        if bins[one[0]] != bins[one[-1]]:
            assert one[::-1] not in legal                                                          # ascending instead of descending
    dead = np.nonzero(~live)[0]
    if dead.size and n_live:
        assert np.concatenate([one[:-1], dead[:1]]) not in legal                                   # a culled tile in the order


# ---------------------------------------------------------------- reorder ----------------------------------------------------------------
def test_reorder_known_answers():
    work = np.array([5, 1, 9, 3, 7, 200, 200], np.uint32)
    order = np.array([0, 1, 2, 3, 4, 6, 5], np.uint32)
    assert list(M.reorder_keys(work, order[:5])) == [114, 227, 0, 170, 57]
    assert list(M.tile_reorder(work, order, [5, 7, 64, 1, 256])) == [2, 4, 0, 3, 1, 6, 5]
    assert list(M.tile_reorder(work, order, [5, 7, 63, 1, 256])) == [2, 1, 4, 3, 0, 6, 5]          # costliest, cheapest, second costliest, second cheapest, middle
    assert list(M.tile_reorder(work, order, [4, 7, 1, 1, 256])) == [2, 1, 0, 3, 4, 6, 5]           # keys of 5, 1, 9, 3: even count
    assert M.deal(list("abcdef")) == list("afbecd") and M.undeal(list("afbecd")) == list("abcdef")
    assert M.reorder_why_not(work, order, [5, 7, 63, 1, 256], [2, 1, 4, 3, 0, 6, 5]) is None
    assert M.reorder_why_not(work, order, [5, 7, 63, 1, 256], [2, 4, 0, 3, 1, 6, 5])               # sorted where dealt is due
    assert M.reorder_why_not(work, order, [5, 7, 64, 1, 256], [2, 1, 4, 3, 0, 6, 5])               # dealt where sorted is due
    assert M.reorder_why_not(work, order, [5, 7, 63, 1, 256], [2, 3, 4, 1, 0, 6, 5])               # dealt one off: cheapest and second cheapest swapped
    assert M.reorder_why_not(work, order, [5, 7, 64, 1, 256], [2, 4, 0, 3, 3, 6, 5])               # a tile twice
    assert M.reorder_why_not(work, order, [5, 7, 64, 1, 256], [2, 4, 0, 3, 1, 5, 6])               # the light part touched


@pytest.mark.parametrize("case", reorder_cases(), ids=lambda c: c[0])
def test_reorder_model_properties(case):
    _, work, order, sched = case
    out = M.tile_reorder(work, order, sched)
    n = sched[0]
    assert M.reorder_why_not(work, order, sched, out) is None
    assert np.array_equal(out[n:], order[n:]) and sorted(out[:n]) == sorted(order[:n])
    w = work[out[:n]].astype(np.int64)
    if n and sched[2] < 64:                                # dealt: the even places run down from the costliest, the odd places up from the cheapest, in key order
        top = max(1, int(w.max()))
        k = 255 - w * 255 // top
        assert (np.diff(k[0::2]) >= 0).all() and (np.diff(k[1::2]) <= 0).all()
        if n >= 2:
            assert k[0] == k.min() and k[1] == k.max()
    elif n:
        assert (np.diff(255 - w * 255 // max(1, int(w.max()))) >= 0).all()
    if n >= 3 and len(set(M.reorder_keys(work, order[:n]))) == n:         # distinct keys: the result is unique, and the other pattern is refused
        other = list(sched)
        other[2] = 64 if sched[2] < 64 else 63
        assert M.reorder_why_not(work, order, other, out) is not None


# ---------------------------------------------------------------- batch table ----------------------------------------------------------------
def test_batch_table_known_answers():
    rows = [[h, h + 5, 64, 8, 32] for h in (0, 1, 7, 8, 9, 17)]
    fields, total = M.batch_table(rows, 64, 1, 250, 128, [0, 300, 600, 900, 1200, 1500])
    assert [b["n_heavy"] for b in fields] == [0, 1, 1, 1, 1, 2, 0, 0, 6, 7, 8, 15]                # the first eighth, at least one, then the rest
    assert [b["n_live"] for b in fields] == [0, 1, 1, 1, 1, 2, 5, 5, 11, 12, 13, 20]
    assert [b["order_base"] for b in fields] == [0, 300, 600, 900, 1200, 1500, 0, 301, 601, 901, 1201, 1502]
    assert all(b["slices"] == 8 and b["chunk_len"] == 32 for b in fields)
    heavy_item, light_item = 64 * 8, 64 * 2                                                        # 2 light slices: ceil(250 / 128)
    ends = np.cumsum([0, 1, 1, 1, 1, 2]) * heavy_item
    assert [b["item_end"] for b in fields[:6]] == list(ends)
    rest = np.cumsum(np.array([0, 0, 6, 7, 8, 15]) * heavy_item + 5 * light_item) + ends[-1]
    assert [b["item_end"] for b in fields[6:]] == list(rest) and total == rest[-1]
    fields0, total0 = M.batch_table(rows, 64, 0, 256, 256, [0] * 6)
    assert all(b["slices"] == 1 and b["chunk_len"] == 256 for b in fields0) and total0 == sum(h + 5 for h in (0, 1, 7, 8, 9, 17)) * 64
    gap, _ = M.batch_table([[12, 20, 64, 16, 16], [0, 0, 64, 64, 4], [3, 3, 64, 8, 32]], 256, 1, 250, 128, [0, 1000, 2000])
    assert gap[1]["item_end"] == gap[0]["item_end"] and gap[4]["item_end"] == gap[3]["item_end"]          # the empty frame owns no item, early or late
    assert (gap[1]["n_live"], gap[4]["n_live"], gap[4]["order_base"]) == (0, 0, 1000)
    big, total = M.batch_table([[100000, 100001, 64, 64, 16]] * 3, 1024, 1, 1000, 128, [0, 200000, 400000])
    assert total == 0xFFFFFFF0 and big[0]["item_end"] == 12500 * 1024 * 64 and [b["item_end"] for b in big[3:]] == [0xFFFFFFF0] * 3


@pytest.mark.parametrize("case", batch_cases(), ids=lambda c: c[0])
def test_batch_table_model_properties(case):
    _, rows, tt, rng_mode, spp, light, base = case
    fields, total = M.batch_table(rows, tt, rng_mode, spp, light, base)
    frames = len(rows)
    ends = [b["item_end"] for b in fields]
    assert ends == sorted(ends) and total == ends[-1]
    for f, row in enumerate(rows):
        a, b = fields[f], fields[frames + f]
        assert a["n_heavy"] + b["n_heavy"] == row[0] and a["n_live"] + b["n_live"] == row[1]     # the two entries split the frame's tiles, none lost
        assert a["n_heavy"] == a["n_live"] == (max(1, row[0] // 8) if row[0] else 0)
        assert (a["order_base"], b["order_base"]) == (base[f], base[f] + a["n_heavy"])
    light_slices = -(-spp // light) if rng_mode == 1 else 1
    exact = sum(r[0] * tt * (r[3] if rng_mode == 1 else 1) + (r[1] - r[0]) * tt * light_slices for r in rows)
    assert total == min(exact, 0xFFFFFFF0)
    words = M.batch_table_words(fields)
    assert set(words) == {15, 16, 17, 18, 19, 20} and all(w.shape == (2 * frames,) for w in words.values())


# ---------------------------------------------------------------- lists ----------------------------------------------------------------
def _disc_frame(W, H, tile):
    """Costs of a frame that sees a disc in its middle, the outermost tile column culled; one legal order and its sched words."""
    yy, xx = np.mgrid[0:H, 0:W]
    hits = (xx - W * 0.45) ** 2 + (yy - H * 0.5) ** 2 < (H * 0.3) ** 2
    t = M.tiling(W, H, tile)
    culled = np.zeros((t["tiles_y"] * tile // 8, t["tiles_x"] * tile // 8), bool)
    culled[:, -(tile // 8):] = True
    cost = M.tile_costs(hits, W, H, tile, culled_blocks=culled)
    bins, sched, legal = M.tile_order(cost, tile, 1, 0, 8)
    return cost, legal.one(), sched, t


@pytest.mark.parametrize("tile", [8, 16, 32])
def test_pixel_lists_model(tile):
    W, H = 97, 61
    cost, order, sched, t = _disc_frame(W, H, tile)
    n_heavy, n_live = sched[0], sched[1]
    assert 0 < n_heavy < n_live < t["mine"]
    tt, bpt = tile * tile, (tile // 8) ** 2
    tile_of = lambda x, row: (row // tile) * t["tiles_x"] + x // tile
    in_tiles = lambda tiles: np.array([[tile_of(x, r) in tiles for x in range(W)] for r in range(H)])
    heavy_px, live_px = in_tiles(set(order[:n_heavy].tolist())), in_tiles(set(order.tolist()))
    light_tile = int(order[n_heavy])
    single = np.zeros((H, W), np.uint8)
    single[(light_tile // t["tiles_x"]) * tile + 3, (light_tile % t["tiles_x"]) * tile + 5] = 1
    edge = np.zeros((H, W), np.uint8)
    edge[:, W - 1] = 1
    edge[H - 1, :] = 1
    masks = {"empty": np.zeros((H, W), np.uint8), "ones": np.ones((H, W), np.uint8), "edge": edge, "single": single,
             "bernoulli": (np.random.default_rng(11).random((H, W)) < 0.3).astype(np.uint8)}
    for name, mask in masks.items():
        words, lh, ll, offs = M.pixel_lists(order, sched, mask, W, H, tile)
        assert words.size == t["mine"] * tt and offs.size == n_live * bpt
        assert lh == int((mask.astype(bool) & heavy_px).sum()) and lh + ll == int((mask.astype(bool) & live_px).sum()), name
        heavy, light = words[:lh], words[n_heavy * tt:n_heavy * tt + ll]
        assert (np.delete(words, np.r_[0:lh, n_heavy * tt:n_heavy * tt + ll]) == M.M32).all()                  # nothing else is written
        both = np.concatenate([heavy, light]).astype(np.int64)
        x, row = both & 0xFFFF, both >> 16
        assert len(set(both.tolist())) == both.size and mask[row, x].all() and (x < W).all() and (row < H).all()
        # in order position, then block, then lane: the sort key of every entry increases along the two lists run together
        pos_of = {int(k): p for p, k in enumerate(order)}
        pos = np.array([pos_of[tile_of(int(a), int(b))] for a, b in zip(x, row)], np.int64)
        sub = ((row % tile) // 8) * (tile // 8) + (x % tile) // 8
        lane = (row % 8) * 8 + x % 8
        key = (pos * bpt + sub) * 64 + lane
        assert (np.diff(key) > 0).all() and (pos[:lh] < n_heavy).all() and (pos[lh:] >= n_heavy).all(), name
        counts = np.bincount(pos * bpt + sub, minlength=n_live * bpt)
        assert np.array_equal(offs, np.concatenate([[0], np.cumsum(counts)[:-1]])), name
    words, lh, ll, _ = M.pixel_lists(order, sched, masks["ones"], W, H, tile)
    assert lh + ll == int(live_px.sum())                                              # all ones: every pixel of every live tile exactly once
    words, lh, ll, _ = M.pixel_lists(order, sched, single, W, H, tile)
    assert (lh, ll) == (0, 1) and int(words[n_heavy * tt]) == ((light_tile % t["tiles_x"]) * tile + 5) | (((light_tile // t["tiles_x"]) * tile + 3) << 16)


def test_host_slices_known_answers():
    assert M.host_slices(256, 0) == (1, 256, 256)
    assert M.host_slices(8, 1) == (8, 1, 128) and M.host_slices(250, 1) == (8, 32, 128) and M.host_slices(7, 1) == (7, 1, 128)
    assert M.host_slices(8, 1, accumulate=True) == (1, 8, 128) and M.host_slices(1000, 1) == (8, 125, 128)
