"""CPU model of the GPU-built linear BVH (csrc/bvh_lbvh.hip, dsrt_host_scene_build_bvh_gpu), bit for bit.

It restates the builder's determinism contract (the header comment of bvh_lbvh.hip), not the kernels' loops:

  bounds    each triangle's box is its vertex min / max; the scene box is the min / max of those; extent = the largest axis span,
            pad = extent * 2^-12 (1e-6 when extent is 0)
  code      centroid 0.5f*(lo+hi) of the UNPADDED box, u = (c - lo_scene) / ext_axis (0 on an axis with no extent), * 2^21, clamped to
            [0, 2^21 - 1], truncated; 21 bits per axis interleaved with x in the top bit of each triple (63 bits)
  pad       after the code: an axis on which the box has zero thickness is widened by pad to either side
  order     a stable sort by code (equal codes keep input order)
  topology  keys extended by their sorted position are all distinct; the range [lo, hi] splits at the one adjacent pair g inside it
            whose common prefix is the shortest; the internal node over [lo, g] is index g, the one over [g + 1, hi] index g + 1;
            the root (node 0) covers everything
  boxes     an internal box is the exact min / max union of its children's; triangle boxes are the padded ones.  min / max order
            -0.0 below +0.0 (what the device's fminf / fmaxf return on gfx950)
  output    a subtree of at most 4 triangles under a kept parent is one leaf (tri_offset = its first sorted position); kept internal
            nodes come first in radix-node order, then the leaves in item order (internal nodes 0..N-2, then triangles 0..N-1)
  sizes     N = 0: no nodes; N <= 4: one leaf over the padded boxes; stack need (height - 1) > 64: DepthError (DSRT_ERR_BVH_DEPTH)

All float arithmetic is float32, as on the device (IEEE division, no contraction).
"""
import numpy as np

NODE_DTYPE = np.dtype([("bbox_min", "<f4", 3), ("bbox_max", "<f4", 3), ("left", "<i4"), ("right", "<i4"), ("tri_offset", "<i4"), ("tri_count", "<i4")])
LEAF_MAX = 4
STACK_MAX = 64
F32 = np.float32


class DepthError(Exception):
    """The tree needs a traversal stack deeper than 64 entries (the library returns DSRT_ERR_BVH_DEPTH)."""

    def __init__(self, height):
        super().__init__(f"stack need {height - 1} > {STACK_MAX}")
        self.height = height


def _key(x):
    """int64 image of float32 values with the float order, -0.0 below +0.0."""
    b = np.asarray(x, F32).view(np.int32).astype(np.int64)
    return np.where(b < 0, b ^ 0x7FFFFFFF, b)


def fmin(a, b):
    return np.where(_key(a) <= _key(b), a, b).astype(F32)


def fmax(a, b):
    return np.where(_key(a) >= _key(b), a, b).astype(F32)


def tri_boxes(verts):
    """verts [N, 3 vertices, 3 axes] float32 -> unpadded lo, hi [N, 3]."""
    v = np.asarray(verts, F32)
    return fmin(fmin(v[:, 0], v[:, 1]), v[:, 2]), fmax(fmax(v[:, 0], v[:, 1]), v[:, 2])


def scene_pad(lo, hi):
    slo, shi = lo.min(axis=0), hi.max(axis=0)          # (the sign of a zero here changes nothing below)
    ext = (shi - slo).astype(F32)
    extent = F32(max(F32(0.0), ext.max()))
    pad = F32(extent * F32(1.0 / 4096.0)) if extent > 0 else F32(1e-6)
    return slo, ext, pad


def spread3(q):
    """21-bit integers -> every third bit of 63, lowest bit at position 0."""
    q = np.asarray(q, np.uint64)
    out = np.zeros_like(q)
    for b in range(21):
        out |= ((q >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b)
    return out


def morton_codes(lo, hi):
    slo, ext, _ = scene_pad(lo, hi)
    c = (F32(0.5) * (lo + hi)).astype(F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.where(ext > 0, ((c - slo).astype(F32) / np.where(ext > 0, ext, F32(1))).astype(F32), F32(0)).astype(F32)
    u = np.minimum(np.maximum((u * F32(2097152.0)).astype(F32), F32(0)), F32(2097151.0))
    q = u.astype(np.uint64)
    return (spread3(q[:, 0]) << np.uint64(2)) | (spread3(q[:, 1]) << np.uint64(1)) | spread3(q[:, 2])


def padded_boxes(lo, hi):
    _, _, pad = scene_pad(lo, hi)
    flat = lo == hi                                     # (-0.0 == +0.0 counts as flat)
    return np.where(flat, lo - pad, lo).astype(F32), np.where(flat, hi + pad, hi).astype(F32)


def _bitlen(x):
    """bit length of non-negative integers < 2^32 (exact through float64)."""
    x = np.asarray(x, np.int64)
    return np.where(x == 0, 0, np.frexp(x.astype(np.float64))[1]).astype(np.int64)


def adjacent_prefix(codes):
    """delta[g] = common-prefix length of sorted keys g and g + 1, each key the 64-bit code followed by its 32-bit position."""
    a, b = codes[:-1], codes[1:]
    x = a ^ b
    hi_w, lo_w = (x >> np.uint64(32)).astype(np.int64), (x & np.uint64(0xFFFFFFFF)).astype(np.int64)
    clz64 = np.where(hi_w != 0, 32 - _bitlen(hi_w), 64 - _bitlen(lo_w))
    g = np.arange(len(a), dtype=np.int64)
    return np.where(x != 0, clz64, 64 + 32 - _bitlen(g ^ (g + 1)))


def radix_topology(codes):
    """codes sorted ascending (uint64, N >= 2) -> children [N-1, 2] (>= 0 internal node, < 0 triangle ~position), ranges [N-1, 2],
    depth [N-1] (root 0).  The split of a range is its adjacent pair of smallest prefix (unique for distinct keys), found with a
    sparse-table range minimum, one level of the tree at a time."""
    n = len(codes)
    delta = adjacent_prefix(codes)
    table = [np.arange(n - 1, dtype=np.int64)]
    while (1 << len(table)) <= n - 1:
        prev, half = table[-1], 1 << (len(table) - 1)
        a, b = prev[:len(prev) - half], prev[half:]
        table.append(np.where(delta[b] < delta[a], b, a))
    children = np.zeros((n - 1, 2), np.int64)
    ranges = np.zeros((n - 1, 2), np.int64)
    depth = np.zeros(n - 1, np.int64)
    node, lo, hi, d = np.array([0]), np.array([0]), np.array([n - 1]), 0
    while node.size:
        # argmin of delta over [lo, hi - 1]
        length = hi - lo
        k = _bitlen(length) - 1
        g = np.empty_like(lo)
        for kk in np.unique(k):
            m = k == kk
            a, b = table[kk][lo[m]], table[kk][hi[m] - 1 - (1 << kk) + 1]
            g[m] = np.where(delta[b] < delta[a], b, a)
        left_internal, right_internal = lo < g, g + 1 < hi
        children[node, 0] = np.where(left_internal, g, ~g)
        children[node, 1] = np.where(right_internal, g + 1, ~(g + 1))
        ranges[node, 0], ranges[node, 1], depth[node] = lo, hi, d
        node = np.concatenate([g[left_internal], (g + 1)[right_internal]])
        lo, hi = np.concatenate([lo[left_internal], (g + 1)[right_internal]]), np.concatenate([g[left_internal], hi[right_internal]])
        d += 1
    return children, ranges, depth


def lbvh_model(verts):
    """verts [N, 3, 3] float32 (triangle, vertex, axis) -> (nodes[NODE_DTYPE], tri_indices int32, height); raises DepthError."""
    verts = np.asarray(verts, F32).reshape(-1, 3, 3)
    n = len(verts)
    if n == 0:
        return np.zeros(0, NODE_DTYPE), np.zeros(0, np.int32), 0
    lo, hi = tri_boxes(verts)
    codes = morton_codes(lo, hi)
    plo, phi = padded_boxes(lo, hi)
    order = np.argsort(codes, kind="stable")
    scodes, slo, shi = codes[order], plo[order], phi[order]             # triangle boxes in sorted position
    if n <= LEAF_MAX:
        nodes = np.zeros(1, NODE_DTYPE)
        blo, bhi = slo[0], shi[0]
        for t in range(1, n):
            blo, bhi = fmin(blo, slo[t]), fmax(bhi, shi[t])
        nodes[0] = (blo, bhi, -1, -1, 0, n)
        return nodes, order.astype(np.int32), 1
    children, ranges, depth = radix_topology(scodes)

    # boxes bottom-up, one level at a time
    ilo, ihi = np.zeros((n - 1, 3), F32), np.zeros((n - 1, 3), F32)
    for d in range(int(depth.max()), -1, -1):
        k = np.flatnonzero(depth == d)
        box = []
        for side in (0, 1):
            c = children[k, side]
            tri = c < 0
            blo = np.where(tri[:, None], slo[np.where(tri, ~c, 0)], ilo[np.where(tri, 0, c)])
            bhi = np.where(tri[:, None], shi[np.where(tri, ~c, 0)], ihi[np.where(tri, 0, c)])
            box.append((blo, bhi))
        ilo[k], ihi[k] = fmin(box[0][0], box[1][0]), fmax(box[0][1], box[1][1])

    # collapse and numbering
    size = ranges[:, 1] - ranges[:, 0] + 1
    keep = size > LEAF_MAX
    parent_internal = np.full(n - 1, -1, np.int64)
    parent_tri = np.full(n, -1, np.int64)
    for side in (0, 1):
        c = children[:, side]
        parent_internal[c[c >= 0]] = np.flatnonzero(c >= 0)
        parent_tri[~c[c < 0]] = np.flatnonzero(c < 0)
    leafroot_int = ~keep & (np.arange(n - 1) != 0) & keep[np.maximum(parent_internal, 0)]
    leafroot_tri = keep[parent_tri]
    leafroot = np.concatenate([leafroot_int, leafroot_tri])
    kidx = np.cumsum(keep) - keep
    lidx = np.cumsum(leafroot) - leafroot
    kept, leaves = int(keep.sum()), int(leafroot.sum())
    nodes = np.zeros(kept + leaves, NODE_DTYPE)

    def ref(c):
        item = np.where(c < 0, (n - 1) + ~c, c)
        return np.where((c >= 0) & keep[np.maximum(c, 0)], kidx[np.maximum(c, 0)], kept + lidx[item])
    k = np.flatnonzero(keep)
    at = kidx[k]
    nodes["bbox_min"][at], nodes["bbox_max"][at] = ilo[k], ihi[k]
    nodes["left"][at], nodes["right"][at] = ref(children[k, 0]), ref(children[k, 1])
    k = np.flatnonzero(leafroot_int)
    at = kept + lidx[k]
    nodes["bbox_min"][at], nodes["bbox_max"][at] = ilo[k], ihi[k]
    nodes["left"][at] = nodes["right"][at] = -1
    nodes["tri_offset"][at], nodes["tri_count"][at] = ranges[k, 0], size[k]
    t = np.flatnonzero(leafroot_tri)
    at = kept + lidx[(n - 1) + t]
    nodes["bbox_min"][at], nodes["bbox_max"][at] = slo[t], shi[t]
    nodes["left"][at] = nodes["right"][at] = -1
    nodes["tri_offset"][at], nodes["tri_count"][at] = t, 1

    # height: levels on the longest root-to-leaf path; a leaf root sits at its radix depth, under kept nodes only
    leaf_depth = np.concatenate([depth[leafroot_int], depth[parent_tri[leafroot_tri]] + 1])
    height = int(leaf_depth.max()) + 1
    if height - 1 > STACK_MAX:
        raise DepthError(height)
    return nodes, order.astype(np.int32), height


def scene_verts(tris):
    """TRI_DTYPE records -> [N, 3, 3] float32 vertices."""
    return np.ascontiguousarray(tris["v"], F32).reshape(-1, 3, 3)
