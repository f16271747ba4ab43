"""Movable rigid bodies: a catalogue of named scenes and pose families beside tests/_bodies_model.py, for the tree shapes its one scene lacks -- more than one
workgroup per launch, a chain of 15 top nodes, several big leaves, empty bodies at every place, trees without a chain, without internal records, of one leaf --
and for the values its three pose sets never produce: -0, boxes flat on every axis, a mirror, subnormal and very large coordinates.

An entry is a list of bodies, each None (empty) or (vertices (k, 3, 3) float32, vertex normals or None for face normals); build() makes the HostScene the way
_bodies_model.build_scene does.  Everything is drawn from fixed seeds.  pack_model() restates, from the node arrays alone, where csrc/scene_pack.hip puts node
records, pair records and big leaves: tests/test_bodies_shapes_host.py proves from it that every entry holds what its row of CATALOGUE's table promises."""
import numpy as np

from _bodies_model import F, SUN, _grid, _pose, _rot, _tris, model_update  # noqa: F401  (model_update, SUN: re-exported for the tests)

# `wide`: the smallest first body with more than 256 movable internal records at one depth AND records deeper still, which come first in the refit list -- so that
# a refit launch of several workgroups starts at an offset (2305 triangles give the first alone: 257 records at the deepest depth).  The host test proves both.
WIDE_BODY, WIDE_SECOND = 4097, 700
SIXTEEN_COUNTS = [12, 5, 7, 20, 9, 6, 11, 13, 8, 15, 17, 5, 19, 10, 7, 14]


# ---- geometry ---------------------------------------------------------------------------------------------------------------------------------------------------

def _soup(rng, k, centre, spread, size):
    """k random triangles of about `size` whose centres lie within `spread` of `centre`."""
    c = np.asarray(centre, np.float64) + rng.uniform(-1, 1, (k, 1, 3)) * np.asarray(spread, np.float64)
    return (c + rng.uniform(-size, size, (k, 3, 3))).astype(F)


def _bent(rng, v):
    """Unit vertex normals that are not the face normals."""
    _, n, _ = _tris(v)
    n = n.astype(np.float64) + rng.uniform(-0.4, 0.4, n.shape)
    return (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(F)


def _coincident(k, centre, step=0.25):
    """k triangles with one common centroid, exactly: (c + a, c + b, c - a - b) with dyadic a, b (body 3 of _bodies_model's scene) -- a leaf of k triangles."""
    cc = np.asarray(centre, np.float64)
    out = []
    for i in range(k):
        a = np.array([step * (i + 1), 0.5, 0.25 * (i % 3)])
        b = np.array([-0.5, step * (i + 2), -0.25 * (i % 2)])
        out.append((cc + a, cc + b, cc - a - b))
    return np.array(out, F)


def _leaf_below_a_node(k, centre, step=0.25):
    """2k triangles: k with one common centroid and k others strung out along +x beyond them, so that the first median split (on x, at k) leaves the coincident
    ones alone in the left half: a big leaf BELOW the body's root."""
    cc = np.asarray(centre, np.float64)
    others = np.concatenate([_grid(cc + (8.0 + 2.0 * i, -0.5, 0.25 * (i % 2)), (1, 0, 0), (0, 1, 0.125), 1, 1)[:1] for i in range(k)])
    return np.concatenate([_coincident(k, centre, step), others.astype(F)])


def _static(rng, k=24):
    return _soup(rng, k, (0.0, 0.0, -3.0), (6.0, 6.0, 0.25), 1.5)


def _entries():
    """{name: [body, ...]} -- see CATALOGUE for what each is for."""
    out = {}
    # wide: a static part, one body of WIDE_BODY triangles, one of WIDE_SECOND
    rng = np.random.default_rng(101)
    big = _soup(rng, WIDE_BODY, (0, 0, 2), (10, 10, 2), 0.3)
    out["wide"] = [(_static(rng), None), (big, _bent(rng, big)), (_soup(rng, WIDE_SECOND, (0, 14, 2), (10, 3, 2), 0.3), None)]
    # sixteen: 16 small bodies on a 4 x 4 grid of places
    rng = np.random.default_rng(102)
    bodies = []
    for b, k in enumerate(SIXTEEN_COUNTS):
        v = _soup(rng, k, (4.0 * (b % 4) - 6.0, 4.0 * (b // 4) - 6.0, 0.5 * (b % 3)), (1.0, 1.0, 0.5), 1.0)
        bodies.append((v, _bent(rng, v) if b % 5 == 2 else None))
    out["sixteen"] = bodies
    # big_leaves: one in the static part (table index 0), 601 triangles directly under the chain, one below an internal node of its body, and an ordinary body
    rng = np.random.default_rng(103)
    c601 = _coincident(601, (0.0, 4.0, 2.0), 1.0 / 64)
    out["big_leaves"] = [(_leaf_below_a_node(9, (-12.0, -6.0, 0.0)), None), (c601, _bent(rng, c601)), (_leaf_below_a_node(11, (-12.0, 0.0, 3.0)), None),
                         (_soup(rng, 8, (6.0, 6.0, 1.0), (1, 1, 1), 1.0), None)]
    rng = np.random.default_rng(104)
    out["empty_static"] = [None, (_soup(rng, 30, (0, 0, 0), (3, 3, 1), 1.0), None), (_soup(rng, 3, (5, 0, 1), (0.5, 0.5, 0.5), 1.0), None)]
    v = _soup(rng, 40, (0, 0, 0), (3, 3, 1), 1.0)
    out["one_live"] = [None, (v, _bent(rng, v))]
    out["one_leaf"] = [None, (_soup(rng, 1, (1, 2, 3), (0, 0, 0), 1.0), None)]
    out["one_leaf_3"] = [None, (_soup(rng, 3, (1, 2, 3), (0.5, 0.5, 0.5), 1.0), None)]
    rng = np.random.default_rng(105)
    out["holes"] = [(_static(rng), None), None, (_soup(rng, 7, (-3, 0, 1), (1, 1, 1), 1.0), None), None, (_soup(rng, 5, (3, 0, 1), (1, 1, 1), 1.0), None), None]
    out["leaves_only"] = [(_static(rng), None)] + [(_soup(rng, k, (3.0 * i - 4.0, 1.0, 1.0), (0.5, 0.5, 0.5), 1.0), None) for i, k in enumerate((4, 1, 3, 2))]
    out["all_empty"] = [(_static(rng), None), None, None]
    # flat_x0: for the minus_zero pose -- body 1 lies in the plane x = 0 around the origin of y and z, so 0 * y and 0 * z take both signs
    out["flat_x0"] = [(_static(rng), None), (_grid((0, -2, -2), (0, 1, 0), (0, 0, 1), 4, 4).astype(F), None)]
    # zero_edge: for the same pose -- body 1 reaches from x = 0 to x = 2 with y < 0 and z < 0 throughout: its vertices at x = 0 are posed to -0, the others to x' < 0,
    # so hi.x of their leaves is -0 before the canonical zero and the box is NOT flat (no pad hides which zero it was)
    out["zero_edge"] = [(_static(rng), None), (_grid((0, -4, -2), (0.5, 0, 0.125), (0, 0.75, 0), 4, 4).astype(F), None)]
    return out


ENTRIES = _entries()
CATALOGUE = sorted(ENTRIES)                  # wide, sixteen, big_leaves, empty_static, one_live, one_leaf (and _3), holes, leaves_only, all_empty; flat_x0 and zero_edge
SPECIAL = [("sixteen", "collapse"), ("big_leaves", "mirror_scale"), ("flat_x0", "minus_zero"), ("zero_edge", "minus_zero"), ("empty_static", "subnormal"), ("one_live", "large")]
CASES = [(name, "rigid") for name in CATALOGUE] + SPECIAL


def build(dsrt, name):
    """HostScene of the entry with its bodies tree, at rest."""
    from dsrt_amd import capi
    mats = np.zeros(2, capi.MAT_DTYPE)
    mats["albedo_tex"] = -1
    mats["albedo"] = [(0.7, 0.7, 0.7), (0.8, 0.5, 0.3)]
    mats["ref_idx"] = 1.5
    hs = dsrt.HostScene()
    for b, body in enumerate(ENTRIES[name]):
        if b:
            assert hs.begin_body() == b
        if body is None:
            continue
        v, n, m = _tris(body[0], body[1], b % 2)
        t = np.zeros(len(v), capi.TRI_DTYPE)
        t["v"], t["n"], t["material_id"], t["albedo_tex"] = v, n, m, -1
        hs.add_arrays(tris=t, mats=mats)
    hs.build_bvh_bodies()
    return hs


def ranges(hs):
    return [hs.body_range(b) for b in range(hs.body_count)]


# ---- poses ------------------------------------------------------------------------------------------------------------------------------------------------------

def _rigid(rng, body):
    """A random rotation about the body's own centre and a short shift: the body stays about where it was."""
    c = np.zeros(3) if body is None else body[0].reshape(-1, 3).astype(np.float64).mean(axis=0)
    R = _rot(rng.standard_normal(3), rng.uniform(0.2, 2.5))
    return _pose(R, c + rng.uniform(-0.5, 0.5, 3) - R @ c)


def poses(name, family="rigid", seed=0):
    """{body: 12 float32} for every body >= 1 of the entry (empty ones included: posing them is legal)."""
    rng = np.random.default_rng([sorted(ENTRIES).index(name), seed])
    bodies = ENTRIES[name]
    out = {b: _rigid(rng, bodies[b]) for b in range(1, len(bodies))}
    special = {"collapse": np.zeros(12, F),
               "mirror_scale": _pose(np.diag([-1.0, 2.0, 0.5]), (0.75, -1.5, 0.25)),
               "minus_zero": np.array([-1, 0, 0, -0.0, 0, 1, 0, 0, 0, 0, 1, 0], F),
               "subnormal": _pose(np.eye(3) * 2.0 ** -140, (0, 0, 0)),
               "large": _pose(np.eye(3), (1e15, 1e15, 1e15))}
    if family == "collapse":                 # every third body: the others keep their rigid poses and stay in the picture
        out.update({b: special[family] for b in out if b % 3 == 0})
    elif family != "rigid":
        out.update({b: special[family] for b in out})
    return out


def runs(p):
    """[(first body, (count, 12) array)] -- the contiguous runs of bodies in a {body: pose}: one set_body_poses call each."""
    out = []
    for b in sorted(p):
        if out and out[-1][0] + len(out[-1][1]) == b:
            out[-1][1].append(p[b])
        else:
            out.append((b, [p[b]]))
    return [(b, np.stack(q).astype(F)) for b, q in out]


def apply(target, p):
    """target.set_body_poses for every run of p; target is a HostScene or a Context."""
    for first, q in runs(p):
        target.set_body_poses(first, q)
    return target


def camera(dsrt, hs, W, H, spp=8, depth=8):
    """A camera that sees the whole of hs (as posed) from above and to the side."""
    pts = hs.arrays()["tris"]["v"].reshape(-1, 3).astype(np.float64)
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    c, r = 0.5 * (lo + hi), max(0.5 * float(np.linalg.norm(hi - lo)), 1.0)
    d = np.array([0.3, -0.8, 1.0]) / np.linalg.norm([0.3, -0.8, 1.0])
    return dsrt.camera_look_at(tuple(c + d * (r / np.tan(np.radians(18.0)))), tuple(c), 40.0, W, H, spp, depth)


# ---- where the upload puts things -------------------------------------------------------------------------------------------------------------------------------

def pack_model(nodes, rngs):
    """csrc/scene_pack.hip's pack_tree, restated on the node array: internal nodes become records in a depth-first walk (left first) and a record's depth is the
    number of internal nodes above it; leaves get ceil(count / 2) pair records each, in the order the records refer to them (left, then right; a tree that is one
    leaf: that leaf); a leaf of more than 7 triangles takes the next entry of the big-leaf table.  Returns a dict:
      record_node, record_depth   per node record
      leaf_pairs                  {leaf node: (first pair record, pair records)}
      big                         [(leaf node, triangles)] in table order
      body_of_node                {node: body}, chain nodes absent
      pairs_of_body               {body: pair records}
      entry_start                 [body] -> movable pair records of the bodies before it (body 1 starts at 0)
      movable_records_at_depth    {depth: internal records of bodies >= 1}"""
    from _bodies_model import chain_and_roots, subtree
    record_node, record_depth, todo = [], [], [(0, 0)]
    while todo:
        k, above = todo.pop()
        if nodes[k]["tri_count"] == 0:
            record_node.append(k)
            record_depth.append(above)
            todo += [(int(nodes[k]["right"]), above + 1), (int(nodes[k]["left"]), above + 1)]
    leaf_pairs, big, next_pair = {}, [], 0
    for k in [c for r in record_node for c in (int(nodes[r]["left"]), int(nodes[r]["right"]))] or [0]:
        cnt = int(nodes[k]["tri_count"])
        if cnt > 0:
            leaf_pairs[k] = (next_pair, (cnt + 1) // 2)
            next_pair += (cnt + 1) // 2
            if cnt > 7:
                big.append((k, cnt))
    _, roots = chain_and_roots(nodes, rngs)
    body_of_node = {k: b for b, root in roots.items() for k in subtree(nodes, root)}
    pairs_of_body = {b: sum(leaf_pairs[k][1] for k, bb in body_of_node.items() if bb == b and k in leaf_pairs) for b in range(len(rngs))}
    entry_start = [0, 0] + list(np.cumsum([pairs_of_body[b] for b in range(1, len(rngs))]))    # [b] for b = 1 .. bodies; [0] is not used
    at_depth = {}
    for k, d in zip(record_node, record_depth):
        if body_of_node.get(k, 0) >= 1:
            at_depth[d] = at_depth.get(d, 0) + 1
    return dict(record_node=record_node, record_depth=record_depth, leaf_pairs=leaf_pairs, big=big, body_of_node=body_of_node, pairs_of_body=pairs_of_body,
                entry_start=[int(e) for e in entry_start], movable_records_at_depth=at_depth)
