"""One validity checker for the non-parity trees (host/bvh_sah.cpp, csrc/bvh_lbvh.hip and the CPU model of the latter, tests/_oracle_lbvh.py)."""
import numpy as np


def flat_pad(verts):
    """host_internal.hpp flat_box_pad: the non-parity builders widen a triangle box that has zero thickness on an axis by this much to either side
    (a leaf box of zero thickness is never hit by the reference's slab test)."""
    ext = np.float32((verts.reshape(-1, 3).max(axis=0) - verts.reshape(-1, 3).min(axis=0)).max())
    return np.float32(ext * np.float32(1.0 / 4096.0)) if ext > 0 else np.float32(1e-6)


def assert_tight(v, nd, pad):
    """Leaf box = the exact float bounds of its triangles, each triangle's own box first widened by `pad` on an axis where it is flat."""
    tri = v.reshape(-1, 3, 3)
    lo, hi = tri.min(axis=1).astype(np.float32), tri.max(axis=1).astype(np.float32)
    flat = lo == hi
    lo = np.where(flat, lo - pad, lo).astype(np.float32)
    hi = np.where(flat, hi + pad, hi).astype(np.float32)
    assert np.array_equal(lo.min(axis=0), nd["bbox_min"]) and np.array_equal(hi.max(axis=0), nd["bbox_max"])
    assert (nd["bbox_max"] > nd["bbox_min"]).all()                        # never a box of zero thickness


def _union_bits(a, b, lower):
    """bits of the min (lower) or max of two float32 triples, ordering -0.0 below +0.0."""
    ka, kb = (np.where(x.view(np.int32) < 0, x.view(np.int32) ^ 0x7FFFFFFF, x.view(np.int32)) for x in (a, b))
    pick_a = ka <= kb if lower else ka >= kb
    return np.where(pick_a, a, b).astype(np.float32).view(np.uint32)


def check_bvh(nodes, idx, verts, stack_need, preorder=False):
    """Every triangle in exactly one leaf of <= 4, every node reached once from the root, each child box inside its parent's, leaf boxes
    tight (assert_tight), and every internal box EQUAL to the union of its children's, bit for bit (-0.0 below +0.0): a box that is too
    large -- stale, or from a wrong split -- fails here although it contains its children.  preorder: internal node n has left == n + 1
    (the host builders' numbering).  stack_need: the scene's, which must be the tree's internal depth and at most 64."""
    n_tris = len(verts)
    assert sorted(idx.tolist()) == list(range(n_tris))                   # a permutation: every triangle in exactly one leaf
    if n_tris == 0:
        assert len(nodes) == 0
        return
    pad = flat_pad(verts)
    seen, covered, deepest = set(), np.zeros(n_tris, bool), 0
    todo = [(0, None, 0)]
    while todo:
        n, parent, above = todo.pop()
        assert n not in seen
        seen.add(n)
        nd = nodes[n]
        if parent is not None:                                            # child box inside the parent's
            assert (nd["bbox_min"] >= nodes[parent]["bbox_min"]).all() and (nd["bbox_max"] <= nodes[parent]["bbox_max"]).all()
        if nd["tri_count"] > 0:
            assert nd["left"] == -1 and nd["right"] == -1 and nd["tri_count"] <= 4
            sl = idx[nd["tri_offset"]:nd["tri_offset"] + nd["tri_count"]]
            assert not covered[sl].any()
            covered[sl] = True
            assert_tight(verts[sl].reshape(-1, 3), nd, pad)
            deepest = max(deepest, above)
        else:
            l, r = int(nd["left"]), int(nd["right"])
            if preorder:
                assert l == n + 1 and r > l                               # pre-order numbering
            assert 0 <= l < len(nodes) and 0 <= r < len(nodes)
            L, R = nodes[l], nodes[r]
            assert np.array_equal(nd["bbox_min"].view(np.uint32), _union_bits(L["bbox_min"], R["bbox_min"], True)), n
            assert np.array_equal(nd["bbox_max"].view(np.uint32), _union_bits(L["bbox_max"], R["bbox_max"], False)), n
            todo += [(r, n, above + 1), (l, n, above + 1)]
    assert covered.all() and len(seen) == len(nodes)
    assert stack_need == deepest and stack_need <= 64
