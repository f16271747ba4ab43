"""CPU model of the scheduling pre-pass (csrc/render_kernel.hip: dsrt_tile_cost_kernel, dsrt_tile_order_kernel, dsrt_tile_reorder_kernel, dsrt_batch_table_kernel,
dsrt_pixel_count / scan / list_kernel; DESIGN.md section 4, "Pre-pass, probe, rng_mode 1, batch").  numpy and Python integers, every value exact.  One function per
stage, each on inputs a test can supply, mirroring the source statement for statement; 32-bit wrap-around is written out (`& M32`) where the source computes in
uint32_t.  Where the kernels leave something open -- the order of tiles inside a bin is whatever order the atomics were served in -- the model returns the SET of
legal results as a checker, not one of them.

Local and global tiles: a shard renders the tiles g with g % shard_count == shard_rank, and its local tile k is global tile g = k * shard_count + shard_rank.  Every
array of the pre-pass is indexed by k.

Culling is OFF -- no block is dropped, every cost word of a tile has bit 31 -- when the scene has spheres (they are tested outside the BVH), in counting builds
(collect_counters != 0), and under DSRT_TUNE_NO_CULLING (a batch: under any of the two low tune flags).  Without a BVH the root test has nothing to test against:
a scene with spheres only is not culled (the first rule), a scene with neither is empty and EVERY block is dropped.  DSRT_TUNE_NATURAL_ORDER has no pre-pass at all.
"""
import numpy as np

M32 = 0xFFFFFFFF
LIVE = 0x80000000                 # bit 31 of a cost word: at least one 8x8 block of the tile is not provably empty
DECIDED_REL = 1e-9                # block_is_culled: a compared dot product is decided when it exceeds this times the product of its operands' norms
PROBE_SPP = 4                     # api_render.hip, kProbeSpp
PROBE_MIN_SPP = 64 * PROBE_SPP    # the probe runs in rng_mode 0 from this many samples per pixel on
BATCH_WORDS = 24                  # sizeof(BatchFrame) / 4 (device_layout.h)
B_ITEM_END, B_ORDER_BASE, B_N_HEAVY, B_N_LIVE, B_SLICES, B_CHUNK_LEN, B_IMAGE_SLOT = 15, 16, 17, 18, 19, 20, 21
SCHED_AT, LIST_LEN_AT, PRE_PAD = 32, 40, 64          # api_render.hip: sched = cost + mine + 32, list_len = sched + 8, pre_stride = mine + 64


# ---- what the host decides before the pre-pass (api_render.hip: make_tiling, plan_render) ----
def tiling(W, H, tile=8, shard_rank=0, shard_count=1):
    count = max(1, shard_count)
    tiles_x, tiles_y = (W + tile - 1) // tile, (H + tile - 1) // tile
    total = tiles_x * tiles_y
    return dict(tile=tile, tiles_x=tiles_x, tiles_y=tiles_y, total=total, mine=(total - shard_rank + count - 1) // count, padded=(total + count - 1) // count)


def host_slices(spp, rng_mode, accumulate=False):
    """(items_per_pixel, chunk_len, light_chunk_len) of dsrt_render / dsrt_render_batch (accumulate: of a sample set of `spp` samples), development switches off."""
    if rng_mode != 1:
        return 1, spp, spp
    chunk_len = (spp + 7) // 8
    if accumulate:
        chunk_len = max(chunk_len, min(spp, 32))
    chunk_len = min(max(chunk_len, 1), 4095)
    return (spp + chunk_len - 1) // chunk_len, chunk_len, min(max(chunk_len, 128), 4095)


def camera12(cam):
    """FrameParams::cam of a GPUCamera: origin, lower-left corner, horizontal, vertical."""
    return np.array([getattr(getattr(cam, f), a) for f in ("origin", "lower_left_corner", "horizontal", "vertical") for a in "xyz"], np.float32)


# ---- dsrt_tile_cost_kernel ----
def block_is_culled(root_lo, root_hi, cam, W, H, x0, ky0):
    """block_footprint_misses_root in float64 for the 8x8 block whose first column is x0 and whose lowest kernel row (ky = H - 1 - image row) is ky0.
    -> (culled, decided).  The comparisons are made in the source's order and with its short circuits (`a = a && (...)`); decided is False when any dot product
    that was compared with zero is within DECIDED_REL * |a| * |b| of it: there a device that rounds differently may decide either way."""
    cam = np.asarray(cam, np.float64)
    o, llc, hor, ver = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
    ulo, uhi = float(x0 - 1) / float(W - 1), float(x0 + 9) / float(W - 1)
    vlo, vhi = float(ky0 - 1) / float(H - 1), float(ky0 + 9) / float(H - 1)
    us, vs = (ulo, uhi, uhi, ulo), (vlo, vlo, vhi, vhi)
    dirs = [(llc + us[c] * hor + vs[c] * ver) - o for c in range(4)]
    mid = np.zeros(3)
    for c in range(4):
        mid = mid + dirs[c]
    lo, hi = np.asarray(root_lo, np.float64), np.asarray(root_hi, np.float64)
    rel = [np.array([(hi[a] if (j >> a) & 1 else lo[a]) - o[a] for a in range(3)]) for j in range(8)]
    decided = True

    def dot(a, b):
        nonlocal decided
        d = a[0] * b[0] + a[1] * b[1] + a[2] * b[2]
        if not abs(d) > DECIDED_REL * np.sqrt(a @ a) * np.sqrt(b @ b):
            decided = False
        return d

    behind = True
    for j in range(8):
        behind = behind and dot(mid, rel[j]) <= 0.0
    if behind:
        return True, decided
    for c in range(4):
        a, b = dirs[c], dirs[(c + 1) & 3]
        n = np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])
        s = dot(n, mid)
        if s == 0.0:
            continue
        if s < 0.0:
            n = -n
        outside = True
        for j in range(8):
            outside = outside and dot(n, rel[j]) < 0.0
        if outside:
            return True, decided
    return False, decided


def frame_culled_blocks(root_lo, root_hi, cam, W, H, tile=8):
    """(culled, decided): one bool per 8x8 block of the TILED frame, [block row][block column], rows from the top -- tiles_y * tile / 8 by tiles_x * tile / 8, so with
    tiles of 16 or 32 including the blocks that lie wholly outside the image: the kernel tests them like any other."""
    t = tiling(W, H, tile)
    rows, cols = t["tiles_y"] * tile // 8, t["tiles_x"] * tile // 8
    culled, decided = np.zeros((rows, cols), bool), np.zeros((rows, cols), bool)
    for br in range(rows):
        for bc in range(cols):
            culled[br, bc], decided[br, bc] = block_is_culled(root_lo, root_hi, cam, W, H, bc * 8, H - 1 - (br * 8 + 7))
    return culled, decided


def tile_costs(hits, W, H, tile, shard_rank=0, shard_count=1, culled_blocks=None):
    """The cost words of a shard's local tiles.  hits: bool (H, W), image rows from the top -- does the pixel's un-jittered centre ray hit anything (an any-hit
    walk and a closest-hit search agree on that).  culled_blocks: frame_culled_blocks()'s first array, or None where culling is off.  A block that is dropped
    ends before it counts, so only the pixels of blocks that are kept are counted (a correct cull drops no pixel that hits)."""
    t = tiling(W, H, tile, shard_rank, shard_count)
    per_row = tile // 8
    cost = np.zeros(t["mine"], np.uint32)
    for k in range(t["mine"]):
        g = k * max(1, shard_count) + shard_rank
        tx, ty = g % t["tiles_x"], g // t["tiles_x"]
        word = 0
        for sub in range(per_row * per_row):
            bx0, brow0 = tx * tile + (sub % per_row) * 8, ty * tile + (sub // per_row) * 8
            if culled_blocks is not None and culled_blocks[brow0 // 8, bx0 // 8]:
                continue
            word |= LIVE
            word += int(hits[brow0:min(H, brow0 + 8), bx0:min(W, bx0 + 8)].sum())        # (pixels beyond the image trace nothing)
        cost[k] = word
    return cost


# ---- dsrt_tile_order_kernel ----
def tile_bin(cost_word, tile):
    """The bin of a live tile, 0 (every pixel sees geometry) ... 64 (fewer than tile^2 / 64 do); -1 for a tile that is not in the order (cost word 0).
    THE BIN RULE: bin = 64 - min(64, pixels * 64 // tile^2) in integers, and the tiles of bin 64 are the LIGHT tiles -- so a 16- or 32-pixel tile that sees
    geometry in fewer than tile^2 / 64 (4 / 16) of its pixels is light, like one that sees none; with 8-pixel tiles light means exactly "sees none"."""
    if cost_word == 0:
        return -1
    full = tile * tile
    return 64 - min(64, (((cost_word & 0x7FFFFFFF) * 64) & M32) // full)


class LegalOrders:
    """The set of orders dsrt_tile_order_kernel may leave: a permutation of exactly the tiles whose cost word is not zero, bins non-decreasing along it; the
    order inside a bin is free."""

    def __init__(self, bins):
        self.bins = np.asarray(bins)
        self.live = np.nonzero(self.bins >= 0)[0]

    def one(self):
        """One member: the live tiles by bin, by tile number inside a bin."""
        return self.live[np.argsort(self.bins[self.live], kind="stable")].astype(np.uint32)

    def why_not(self, order):
        order = np.asarray(order, np.int64)
        if order.size != self.live.size:
            return f"{order.size} entries for {self.live.size} live tiles"
        if order.size and (order.min() < 0 or order.max() >= self.bins.size):
            return "an entry is no tile"
        if not np.array_equal(np.sort(order), self.live):
            return "not a permutation of the live tiles (a tile twice, a tile missing or a culled tile)"
        b = self.bins[order]
        if (np.diff(b) < 0).any():
            return f"bins decrease at position {int(np.nonzero(np.diff(b) < 0)[0][0]) + 1}"
        return None

    def __contains__(self, order):
        return self.why_not(order) is None


def tile_order(cost, tile, items_per_pixel, resident_lanes, spp):
    """-> (bins per tile, sched[0..4] as Python ints, LegalOrders).  sched: [0] n_heavy = live tiles in bins 0..63, [1] n_live, [2] spread, [3] slices, [4] chunk_len."""
    cost = [int(c) for c in np.asarray(cost, np.uint32)]
    full = tile * tile
    bins = np.array([tile_bin(c, tile) for c in cost], np.int64)
    acc = int((bins >= 0).sum())
    n_heavy = acc - int((bins == 64).sum())
    slices, chunk_len = items_per_pixel, spp
    if items_per_pixel > 1:
        heavy_pixels = n_heavy * full
        while slices < 64 and ((slices * 2) & M32) <= spp and heavy_pixels * slices * 2 <= resident_lanes:
            slices = (slices * 2) & M32
        chunk_len = ((spp + slices - 1) & M32) // slices
        slices = ((spp + chunk_len - 1) & M32) // chunk_len
    heavy_items = n_heavy * full * slices
    spread = 64
    if heavy_items < resident_lanes:
        spread = ((heavy_items * 64 + resident_lanes - 1) // resident_lanes) & M32
    return bins, [n_heavy, acc, 1 if spread < 1 else spread, slices, chunk_len], LegalOrders(bins)


# ---- dsrt_tile_reorder_kernel ----
def reorder_keys(work, tiles):
    """The 256-bin key of every tile of `tiles` (the heavy part of an order): 255 - work * 255 // max(1, the largest work among them)."""
    w = [int(work[int(t)]) for t in tiles]
    top = max([1] + w)
    return np.array([255 - v * 255 // top for v in w], np.int64)


def deal(seq):
    """costliest, cheapest, second costliest, second cheapest, ...: position i takes seq[i >> 1] when i is even and seq[n - 1 - (i >> 1)] when it is odd."""
    n = len(seq)
    return [seq[n - 1 - (i >> 1)] if i & 1 else seq[i >> 1] for i in range(n)]


def undeal(seq):
    n = len(seq)
    out = [None] * n
    for i in range(n):
        out[n - 1 - (i >> 1) if i & 1 else i >> 1] = seq[i]
    return out


def tile_reorder(work, order, sched):
    """One legal result: the first sched[0] entries sorted by key (stable, where the kernel's order inside a key is free), dealt when sched[2] < 64; the rest untouched."""
    order = [int(t) for t in order]
    n = int(sched[0])
    keys = reorder_keys(work, order[:n])
    head = [order[i] for i in np.argsort(keys, kind="stable")]
    if int(sched[2]) < 64:
        head = deal(head)
    return np.array(head + order[n:], np.uint32)


def reorder_why_not(work, order_in, sched, order_out):
    """None when order_out is a result dsrt_tile_reorder_kernel may leave for (work, order_in, sched), else what is wrong with it."""
    order_in, order_out = [int(t) for t in order_in], [int(t) for t in order_out]
    n = int(sched[0])
    if len(order_out) != len(order_in):
        return "length changed"
    if order_out[n:] != order_in[n:]:
        return "entries from sched[0] on were touched"
    if sorted(order_out[:n]) != sorted(order_in[:n]):
        return "the heavy part is not a permutation of itself"
    head = undeal(order_out[:n]) if int(sched[2]) < 64 else order_out[:n]
    keys = reorder_keys(work, head)
    if (np.diff(keys) < 0).any():
        return ("dealt: the sequence dealt from" if int(sched[2]) < 64 else "sorted: the sequence") + f" has keys that decrease at position {int(np.nonzero(np.diff(keys) < 0)[0][0]) + 1}"
    return None


# ---- dsrt_batch_table_kernel ----
def batch_table(sched, tt, rng_mode, spp, light_chunk_len, order_base):
    """sched: per frame its five sched words.  -> (fields, total): fields[e] = dict of the words the kernel writes in entry e of 2 * frames (entry f: the first
    eighth of frame f's heavy tiles, at least one of them; entry frames + f: the rest, its order_base moved on by that many), total = the last item_end."""
    frames = len(sched)
    acc = 0
    light_slices = (spp + light_chunk_len - 1) // light_chunk_len if rng_mode == 1 else 1
    sat = lambda v: 0xFFFFFFF0 if v > 0xFFFFFFF0 else v
    out = []
    for e in range(2 * frames):
        f = e if e < frames else e - frames
        n_heavy, n_live = int(sched[f][0]), int(sched[f][1])
        top = ((n_heavy >> 3) if (n_heavy >> 3) else 1) if n_heavy else 0
        b = dict(order_base=int(order_base[f]))
        if e < frames:
            b["n_heavy"], b["n_live"] = top, top
        else:
            b["n_heavy"], b["n_live"], b["order_base"] = (n_heavy - top) & M32, (n_live - top) & M32, (b["order_base"] + top) & M32
        b["slices"] = int(sched[f][3]) if rng_mode == 1 else 1
        b["chunk_len"] = int(sched[f][4]) if rng_mode == 1 else spp
        acc += b["n_heavy"] * tt * b["slices"] + ((b["n_live"] - b["n_heavy"]) & M32) * tt * light_slices
        b["item_end"] = sat(acc)
        out.append(b)
    return out, sat(acc)


def batch_table_words(fields):
    """The words of batch_table()'s fields where they lie in a BatchFrame: (entries, 7) columns B_ITEM_END ... B_CHUNK_LEN are indices into the 24 words."""
    cols = (("item_end", B_ITEM_END), ("order_base", B_ORDER_BASE), ("n_heavy", B_N_HEAVY), ("n_live", B_N_LIVE), ("slices", B_SLICES), ("chunk_len", B_CHUNK_LEN))
    return {at: np.array([b[name] for b in fields], np.uint32) for name, at in cols}


# ---- dsrt_pixel_count / scan / list_kernel ----
def pixel_lists(order, sched, mask, W, H, tile):
    """The lists of a masked launch (one shard: the whole frame).  mask: (H, W), nonzero = active.  -> (words, len_heavy, len_light, offsets): `words` has
    mine * tile^2 entries, 0xFFFFFFFF where the kernels write nothing -- the heavy list from 0, the light list from n_heavy * tile^2, each entry x | row << 16,
    in order position, then 8x8 block of the tile (row-major), then lane (x = lane & 7, row = lane >> 3); offsets: per block of every live tile in that order, the
    number of active pixels before it, counted through both lists."""
    t = tiling(W, H, tile)
    per_row, tt = tile // 8, tile * tile
    n_heavy, n_live = int(sched[0]), int(sched[1])
    words = np.full(t["mine"] * tt, M32, np.uint32)
    offsets = np.zeros(n_live * per_row * per_row, np.uint32)
    heavy, light, run = [], [], 0
    for pos in range(n_live):
        k = int(order[pos])
        for sub in range(per_row * per_row):
            offsets[pos * per_row * per_row + sub] = run
            for lane in range(64):
                x, row = (k % t["tiles_x"]) * tile + (sub % per_row) * 8 + (lane & 7), (k // t["tiles_x"]) * tile + (sub // per_row) * 8 + (lane >> 3)
                if x < W and row < H and mask[row, x]:
                    (heavy if pos < n_heavy else light).append(x | (row << 16))
                    run += 1
    words[:len(heavy)] = heavy
    words[n_heavy * tt:n_heavy * tt + len(light)] = light
    return words, len(heavy), len(light), offsets


# ---- the pre-pass's input from the oracle ----
def centre_hits(oracle_lib, scene, W, H):
    """bool (H, W), image rows from the top: does the centre ray of the pixel -- dsrt_oracle_camera_ray at jitter (0.5, 0.5) -- hit anything, spheres included, in
    dsrt_oracle_scene_hit with the renderer's t_min = 0.001 and t_max = 1e9 (device_math.h, kTMin / kTMax)."""
    import ctypes as C
    L = oracle_lib
    L.dsrt_oracle_camera_ray.restype = None
    L.dsrt_oracle_camera_ray.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    o3, d3, out, ids = (C.c_float * 3)(), (C.c_float * 3)(), (C.c_float * 9)(), (C.c_int * 4)()
    hits = np.zeros((H, W), bool)
    sp, cam = C.byref(scene), C.byref(scene.camera)
    for r in range(H):
        for x in range(W):
            L.dsrt_oracle_camera_ray(cam, x, H - 1 - r, W, H, 0.5, 0.5, o3, d3)
            hits[r, x] = bool(L.dsrt_oracle_scene_hit(sp, o3, d3, 0.001, 1e9, out, ids))
    return hits
