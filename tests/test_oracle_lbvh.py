"""The CPU model of the GPU-built LBVH (tests/_oracle_lbvh.py) checked on its own, without a GPU: its topology against a literal
restatement of Karras 2012 section 4, its Morton codes against a bit-by-bit interleave, and its trees through the shared validity checker
(tests/_bvh_check.py), which holds every internal box to the exact union of its children.  tests/test_gpu_lbvh.py then holds the
device's output to this model byte for byte."""
import os

import numpy as np
import pytest

import _lbvh_scenes as S
from _bvh_check import check_bvh
from _oracle_lbvh import (NODE_DTYPE, DepthError, adjacent_prefix, lbvh_model, morton_codes, padded_boxes, radix_topology, scene_pad,
                          tri_boxes)
from conftest import ASSETS

F = np.float32


def _karras(keys):
    """radix_tree_kernel of csrc/bvh_lbvh.hip restated literally: the doubling search for the far end, the binary search for the split."""
    n = len(keys)
    keys = [int(k) for k in keys]

    def lcp(i, j):
        if j < 0 or j >= n:
            return -1
        a, b = keys[i], keys[j]
        return 64 - (a ^ b).bit_length() if a != b else 64 + 32 - (i ^ j).bit_length()
    children = []
    for i in range(n - 1):
        d = 1 if lcp(i, i + 1) - lcp(i, i - 1) > 0 else -1
        floor = lcp(i, i - d)
        reach = 2
        while lcp(i, i + reach * d) > floor:
            reach <<= 1
        length, t = 0, reach >> 1
        while t > 0:
            if lcp(i, i + (length + t) * d) > floor:
                length += t
            t >>= 1
        j = i + length * d
        node = lcp(i, j)
        s, div = 0, 2
        t = (length + 1) // 2
        while True:
            if lcp(i, i + (s + t) * d) > node:
                s += t
            if t <= 1:
                break
            div <<= 1
            t = (length + div - 1) // div
        g = i + s * d + (-1 if d < 0 else 0)
        lo, hi = min(i, j), max(i, j)
        children.append((~g if lo == g else g, ~(g + 1) if hi == g + 1 else g + 1))
    return np.array(children, np.int64).reshape(-1, 2)


def _key_sets():
    rng = np.random.default_rng(7)
    out = {"random_2000": np.sort(rng.integers(0, 1 << 63, 2000, dtype=np.uint64))}
    runs = np.sort(rng.integers(0, 40, 1500)).astype(np.uint64) << np.uint64(50)     # long runs of equal codes
    out["runs_1500"] = runs
    out["all_equal_1000"] = np.full(1000, 12345, np.uint64)
    out["all_equal_5"] = np.zeros(5, np.uint64)
    out["two"] = np.array([3, 9], np.uint64)
    out["small_spread"] = np.sort(rng.integers(0, 8, 700)).astype(np.uint64)
    out["top_bits"] = np.sort(np.array([(1 << 62) | k for k in range(300)] + [k << 40 for k in range(300)], np.uint64))
    return out


@pytest.mark.parametrize("name", sorted(_key_sets()))
def test_model_topology_is_karras_section_4(name):
    keys = _key_sets()[name]
    children, ranges, depth = radix_topology(keys)
    assert np.array_equal(children, _karras(keys))
    assert (ranges[0] == [0, len(keys) - 1]).all() and depth[0] == 0


def test_adjacent_prefix_uses_position_for_equal_codes():
    keys = np.array([5, 5, 5, 5, 6], np.uint64)
    # 5 ^ 6 = 3: 62 leading zeros; equal codes continue into the 32-bit positions (0^1, 1^2, 2^3)
    assert adjacent_prefix(keys).tolist() == [64 + 31, 64 + 30, 64 + 31, 62]


def _interleave(qx, qy, qz):
    code = 0
    for b in range(20, -1, -1):
        code = (code << 3) | (((qx >> b) & 1) << 2) | (((qy >> b) & 1) << 1) | ((qz >> b) & 1)
    return code


def test_morton_codes_against_a_bit_by_bit_interleave():
    verts = S.random_tris(500, 11)
    lo, hi = tri_boxes(verts)
    codes = morton_codes(lo, hi)
    slo, ext, _ = scene_pad(lo, hi)
    for i in range(0, 500, 7):
        q = []
        for a in range(3):
            c = F(F(0.5) * F(lo[i, a] + hi[i, a]))
            u = F(F(c - slo[a]) / ext[a])
            q.append(int(min(max(F(u * F(2097152.0)), F(0.0)), F(2097151.0))))
        assert int(codes[i]) == _interleave(*q), i
    # the ends: the scene's lower corner is code 0, its upper corner all 63 bits (the clamp at 2^21 - 1)
    pts = S.one_point(1, (0.0, 0.0, 0.0)).tolist() + S.one_point(1, (2.0, 4.0, 8.0)).tolist() + S.one_point(1, (1.0, 0.0, 8.0)).tolist()
    lo, hi = tri_boxes(np.array(pts, F))
    assert morton_codes(lo, hi).tolist() == [0, (1 << 63) - 1, _interleave(1 << 20, 0, (1 << 21) - 1)]


def test_flat_pad_follows_the_code_and_uses_the_scene_extent():
    verts = S.quad(0.25, 1.0, 2)                                          # extent 2 on x and y, 0 on z
    lo, hi = tri_boxes(verts)
    plo, phi = padded_boxes(lo, hi)
    pad = F(2.0 / 4096.0)
    assert (plo[:, 2] == F(F(0.25) - pad)).all() and (phi[:, 2] == F(F(0.25) + pad)).all()
    assert np.array_equal(plo[:, :2], lo[:, :2])
    lo, hi = tri_boxes(S.one_point(3))
    plo, phi = padded_boxes(lo, hi)                                       # a scene of one point: extent 0, pad 1e-6
    assert (plo == np.array([1.5, -2.0, 0.25], F) - F(1e-6)).all() and (phi == np.array([1.5, -2.0, 0.25], F) + F(1e-6)).all()


def test_node_dtype_is_the_library_layout(dsrt):
    assert NODE_DTYPE == dsrt.capi.NODE_DTYPE


@pytest.mark.parametrize("name", sorted(S.synthetic_cases()))
def test_model_trees_are_valid(name):
    verts = S.synthetic_cases()[name]
    try:
        nodes, idx, height = lbvh_model(verts)
    except DepthError:
        assert name.startswith("nested_")
        return
    if name.startswith("ulp_cluster"):                                   # (a pad below half an ulp leaves a flat box flat: none here)
        assert (nodes["bbox_max"] > nodes["bbox_min"]).all()
    check_bvh(nodes, idx, verts, height - 1)
    n = len(verts)
    assert np.array_equal(idx, np.argsort(morton_codes(*tri_boxes(verts)), kind="stable"))
    if n <= 4:
        assert len(nodes) == 1 and nodes[0]["tri_count"] == n
    else:
        leaves = nodes["tri_count"] > 0
        assert leaves.sum() >= 2 and (nodes["tri_count"][~leaves] == 0).all() and not leaves[0]
        first_leaf = int(np.argmax(leaves))
        assert not leaves[:first_leaf].any() and leaves[first_leaf:].all()   # kept internal nodes first, then the leaves


def test_nested_cases_reach_both_sides_of_the_depth_limit():
    outcome = {}
    for name, verts in S.synthetic_cases().items():
        if name.startswith("nested_"):
            try:
                outcome[name] = lbvh_model(verts)[2] - 1
            except DepthError as e:
                outcome[name] = e.height - 1
    assert any(v > 64 for v in outcome.values()) and any(v <= 64 for v in outcome.values()), outcome
    assert any(55 <= v <= 64 for v in outcome.values()), outcome                # a tree close to the limit that still builds


def test_small_flat_scenes_get_padded_single_leaves():
    """The N <= 4 path: a quad in the plane z = 0.25 is one leaf whose box has thickness 2 * extent / 4096 on z."""
    nodes, idx, height = lbvh_model(S.quad(0.25, 1.0, 2))
    assert height == 1 and len(nodes) == 1
    assert nodes[0]["bbox_min"][2] < F(0.25) < nodes[0]["bbox_max"][2]


def test_signed_zero_faces_keep_minus_zero_on_the_lower_face():
    nodes, _, _ = lbvh_model(S.small_signed_zeros())
    assert nodes[0]["bbox_min"][0].view(np.uint32) == 0x80000000          # min(-0.0, +0.0) is -0.0


@pytest.mark.parametrize("world", ["station_3k", "mixed", "textured", "quirks", "lights", "c1_spheres"])
def test_model_trees_of_the_parity_worlds_are_valid(dsrt, world):
    cwd = os.getcwd()
    os.chdir(ASSETS)
    try:
        hs = dsrt.HostScene().add_world_file(world + ".world")
    finally:
        os.chdir(cwd)
    hs.build_bvh("sah")
    verts = hs.arrays()["tris"]["v"]
    nodes, idx, height = lbvh_model(verts)
    check_bvh(nodes, idx, verts, height - 1)


def test_model_is_fast_enough_for_a_large_mesh():
    """The GPU file models the 1M-triangle station; the model works level by level, not node by node."""
    import time
    verts = S.random_tris(200000, 3, size=0.01)
    t0 = time.perf_counter()
    nodes, idx, height = lbvh_model(verts)
    assert time.perf_counter() - t0 < 10.0
    assert len(nodes) > 200000 // 4 and height <= 65
