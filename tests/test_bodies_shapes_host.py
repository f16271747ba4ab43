"""Movable rigid bodies on the host, on the catalogue of tests/_bodies_shapes.py: dsrt_host_scene_set_body_poses against the numpy model of tests/_bodies_model.py
bit for bit on every entry and pose family, and the proof -- from the node arrays and from where the upload puts records -- that every entry holds the shape it is
there for.  tests/test_gpu_bodies_shapes.py then holds the device to the host form on the same cases."""
import numpy as np
import pytest

import _bodies_model as M
import _bodies_shapes as S

F, U = np.float32, np.uint32


def _bits(a):
    return np.ascontiguousarray(a, F).view(U)


def _assert_is_model(hs, rest, rngs, poses):
    got = hs.arrays()
    v, n, lo, hi = M.model_update(rest["tris"], got["nodes"], got["idx"], rngs, poses)
    assert np.array_equal(_bits(got["tris"]["v"]), _bits(v)), "vertices"
    assert np.array_equal(_bits(got["tris"]["n"]), _bits(n)), "normals"
    assert np.array_equal(_bits(got["nodes"]["bbox_min"]), _bits(lo)) and np.array_equal(_bits(got["nodes"]["bbox_max"]), _bits(hi)), "node boxes"
    for k in ("uv", "material_id", "albedo_tex"):
        assert np.array_equal(got["tris"][k], rest["tris"][k])
    for k in ("left", "right", "tri_offset", "tri_count"):
        assert np.array_equal(got["nodes"][k], rest["nodes"][k])                               # the topology is fixed
    assert np.array_equal(got["idx"], rest["idx"])
    return got


@pytest.mark.parametrize("name, family", S.CASES)
def test_host_update_is_the_model_bit_for_bit(dsrt, name, family):
    hs = S.build(dsrt, name)
    rest, rngs = hs.arrays(), S.ranges(hs)
    _assert_is_model(hs, rest, rngs, {})                                                       # at rest
    p = S.poses(name, family)
    assert sorted(p) == list(range(1, len(S.ENTRIES[name])))
    got = _assert_is_model(S.apply(hs, p), rest, rngs, p)
    assert np.isfinite(got["tris"]["v"]).all() and np.isfinite(got["nodes"]["bbox_min"]).all() and np.isfinite(got["nodes"]["bbox_max"]).all()
    if len(p) > 1:                                                                             # one body alone, on a fresh scene: the others stay at rest
        b = max(p)
        _assert_is_model(S.build(dsrt, name).set_body_poses(b, p[b][None]), rest, rngs, {b: p[b]})


def _structure(dsrt, name):
    hs = S.build(dsrt, name)
    a, rngs = hs.arrays(), S.ranges(hs)
    chain, roots = M.chain_and_roots(a["nodes"], rngs)
    return hs, a, rngs, chain, roots, S.pack_model(a["nodes"], rngs)


def test_catalogue_is_what_the_cases_need(dsrt):
    for name in S.CATALOGUE:                                                                   # the pack model's own bookkeeping, on every entry
        hs, a, rngs, chain, roots, pk = _structure(dsrt, name)
        nodes = a["nodes"]
        assert [n for _, n in rngs] == [0 if b is None else len(b[0]) for b in S.ENTRIES[name]]
        assert len(pk["record_node"]) == int((nodes["tri_count"] == 0).sum()) and len(pk["leaf_pairs"]) == int((nodes["tri_count"] > 0).sum())
        assert sum(pk["pairs_of_body"].values()) == sum(n for _, n in pk["leaf_pairs"].values())
        assert hs.stack_need == max([d + 1 for d in pk["record_depth"]] + [0])
        if name in ("wide", "sixteen", "big_leaves", "one_live"):                             # a few bodies whose vertex normals are not the face normals
            assert not np.array_equal(a["tris"]["n"], M._tris(a["tris"]["v"])[1])

    # wide: more than one workgroup in the transform launch and in one refit launch, and launches that start beyond entry 256
    hs, a, rngs, chain, roots, pk = _structure(dsrt, "wide")
    assert len(rngs) == 3 and rngs[0][1] > 0 and [n for _, n in rngs[1:]] == [S.WIDE_BODY, S.WIDE_SECOND]
    assert pk["pairs_of_body"][1] > 256 and pk["pairs_of_body"][2] > 256
    assert pk["entry_start"][2] > 256 and pk["entry_start"][2] % 256 != 0                      # body 2 alone: `first` > 256 and not on a block boundary

    def wide_launch_at_an_offset(at):                                                          # a depth of more than 256 movable records with deeper ones before it in the refit list
        return any(n > 256 and any(e > d for e in at) for d, n in at.items())
    assert wide_launch_at_an_offset(pk["movable_records_at_depth"])

    def one_fewer():                                                                           # the same scene with body 1 a triangle short
        keep = S.ENTRIES["wide"]
        try:
            S.ENTRIES["wide"] = [keep[0], (keep[1][0][:-1], keep[1][1][:-1]), keep[2]]
            h = S.build(dsrt, "wide")
            return S.pack_model(h.arrays()["nodes"], S.ranges(h))["movable_records_at_depth"]
        finally:
            S.ENTRIES["wide"] = keep
    assert not wide_launch_at_an_offset(one_fewer())                                           # the smallest such body

    # sixteen: a chain of 15, every body live, odd counts among them
    hs, a, rngs, chain, roots, pk = _structure(dsrt, "sixteen")
    assert len(rngs) == dsrt.capi.MAX_BODIES == 16 and len(chain) == 15 and sorted(roots) == list(range(16))
    assert all(5 <= n <= 20 for _, n in rngs) and sum(n % 2 for _, n in rngs) >= 4
    assert len({tuple(S.poses("sixteen")[b]) for b in range(1, 16)}) == 15                     # every body its own pose

    # big_leaves: at least three, the static one first in the table, 601 triangles in one, one below an internal node of its body
    hs, a, rngs, chain, roots, pk = _structure(dsrt, "big_leaves")
    nodes = a["nodes"]
    big_body = [pk["body_of_node"][k] for k, _ in pk["big"]]
    assert len(pk["big"]) >= 3 and big_body[0] == 0 and all(b >= 1 for b in big_body[1:])      # the movable ones are not index 0 of the table
    assert [cnt for _, cnt in pk["big"]] == [9, 601, 11]
    assert roots[1] == pk["big"][1][0] and pk["leaf_pairs"][roots[1]][1] == 301                # directly under the chain: 301 pair records in the chain lane's loop
    below = pk["big"][2][0]
    assert below != roots[2] and nodes[roots[2]]["tri_count"] == 0 and int(nodes[roots[2]]["left"]) == below   # ... and under an internal node: the refit kernel's
    for k, cnt in pk["big"]:
        tri = a["tris"]["v"][a["idx"][nodes[k]["tri_offset"]:nodes[k]["tri_offset"] + cnt]]
        cen = (tri[:, 0] + tri[:, 1] + tri[:, 2]) / F(3.0)
        assert (_bits(cen) == _bits(cen[0])).all()                                             # one common centroid, exactly

    # the trees without a chain, without internal records, with holes
    hs, a, rngs, chain, roots, pk = _structure(dsrt, "empty_static")
    assert rngs[0][1] == 0 and len(chain) == 1 and sorted(roots) == [1, 2] and a["nodes"][roots[2]]["tri_count"] == 3 and a["nodes"][roots[1]]["tri_count"] == 0
    hs, a, rngs, chain, roots, pk = _structure(dsrt, "one_live")
    assert rngs[0][1] == 0 and chain == [] and roots == {1: 0} and a["nodes"][0]["tri_count"] == 0 and 35 <= rngs[1][1] <= 45
    for name, k in (("one_leaf", 1), ("one_leaf_3", 3)):
        hs, a, rngs, chain, roots, pk = _structure(dsrt, name)
        assert rngs == [(0, 0), (0, k)] and chain == [] and len(a["nodes"]) == 1 and a["nodes"][0]["tri_count"] == k       # the whole tree is one leaf
        assert pk["record_node"] == [] and pk["leaf_pairs"] == {0: (0, (k + 1) // 2)}
    hs, a, rngs, chain, roots, pk = _structure(dsrt, "holes")
    assert [n for _, n in rngs] == [rngs[0][1], 0, 7, 0, 5, 0] and rngs[0][1] > 0 and sorted(roots) == [0, 2, 4] and len(chain) == 2
    assert pk["entry_start"][1] == pk["entry_start"][2] == 0 and pk["entry_start"][3] == pk["entry_start"][4] and pk["entry_start"][5] == pk["entry_start"][6]
    hs, a, rngs, chain, roots, pk = _structure(dsrt, "leaves_only")
    assert rngs[0][1] > 0 and [n for _, n in rngs[1:]] == [4, 1, 3, 2] and all(a["nodes"][roots[b]]["tri_count"] == rngs[b][1] for b in (1, 2, 3, 4))
    assert pk["movable_records_at_depth"] == {} and len(chain) == 4                            # an empty refit list
    hs, a, rngs, chain, roots, pk = _structure(dsrt, "all_empty")
    assert [n for _, n in rngs[1:]] == [0, 0] and sorted(roots) == [0] and chain == [] and pk["pairs_of_body"][1] == pk["pairs_of_body"][2] == 0

    # the values: -0, subnormals, flat on every axis, a mirror, large
    def posed(name, family):
        h = S.build(dsrt, name)
        rest, rngs = h.arrays(), S.ranges(h)
        return rest, rngs, S.apply(h, S.poses(name, family)).arrays()
    rest, rngs, got = posed("flat_x0", "minus_zero")
    first, cnt = rngs[1]
    x = _bits(got["tris"]["v"][first:first + cnt, :, 0])
    assert (x == 0x80000000).any() and (x == 0).any() and np.isin(x, (0, 0x80000000)).all()    # -0 and +0 among the posed x, nothing else
    _, roots = M.chain_and_roots(got["nodes"], rngs)
    pad = M.body_pad(rest["tris"]["v"][first:first + cnt])
    for k in M.subtree(got["nodes"], roots[1]):                                                # every box of the body: +0 -/+ pad in x, whichever zero fminf returned
        assert _bits(got["nodes"][k]["bbox_min"][0]) == _bits(F(0.0) - pad) and _bits(got["nodes"][k]["bbox_max"][0]) == _bits(F(0.0) + pad)
    rest, rngs, got = posed("zero_edge", "minus_zero")
    first, cnt = rngs[1]
    x = got["tris"]["v"][first:first + cnt, :, 0]
    assert (_bits(x) == 0x80000000).any() and not (_bits(x) == 0).any() and (x <= 0).all() and (x < 0).any()     # -0 is the largest posed x, and +0 is not among them
    _, roots = M.chain_and_roots(got["nodes"], rngs)
    hi_x = np.array([got["nodes"][k]["bbox_max"][0] for k in M.subtree(got["nodes"], roots[1])])
    lo_x = np.array([got["nodes"][k]["bbox_min"][0] for k in M.subtree(got["nodes"], roots[1])])
    assert (_bits(hi_x) == 0).any() and not (_bits(hi_x) == 0x80000000).any() and (lo_x[_bits(hi_x) == 0] < 0).all()   # boxes that end at +0, not flat: only the canonical zero made them so
    rest, rngs, got = posed("empty_static", "subnormal")
    v = got["tris"]["v"]
    tiny = np.abs(v) < np.finfo(F).tiny
    assert tiny.all() and (v != 0).all(axis=(1, 2)).any() and (v != 0).any(axis=(1, 2)).all()  # subnormal everywhere, no triangle flushed to zero
    assert (got["nodes"]["bbox_max"] > got["nodes"]["bbox_min"]).all()
    rest, rngs, got = posed("sixteen", "collapse")
    _, roots = M.chain_and_roots(got["nodes"], rngs)
    for b in range(3, 16, 3):
        first, cnt = rngs[b]
        assert not got["tris"]["v"][first:first + cnt].any() and not got["tris"]["n"][first:first + cnt].any()
        pad = M.body_pad(rest["tris"]["v"][first:first + cnt])
        for k in M.subtree(got["nodes"], roots[b]):
            if got["nodes"][k]["tri_count"] > 0:                                               # flat on all three axes, padded on all three
                assert (got["nodes"][k]["bbox_min"] == -pad).all() and (got["nodes"][k]["bbox_max"] == pad).all()
    rest, rngs, got = posed("big_leaves", "mirror_scale")
    first, cnt = rngs[1]
    assert np.array_equal(got["tris"]["v"][first:first + cnt, :, 1], F(2.0) * rest["tris"]["v"][first:first + cnt, :, 1] + F(-1.5))
    rest, rngs, got = posed("one_live", "large")
    assert (got["tris"]["v"] > 9e14).all() and np.isfinite(got["nodes"]["bbox_max"]).all()
