"""Movable rigid bodies (include/dsrt.h, MOVABLE RIGID BODIES): the test scene, the pose sets, and a numpy float32 model of the arithmetic of a pose update.

The model states the header's rules once more, independently of host/bvh_bodies.cpp and csrc/bodies_kernel.hip: every numpy operation below is one correctly
rounded float32 operation, in the order the header writes it.  It takes the tree's TOPOLOGY (children, leaf ranges, tri_indices) from the library -- that is
pinned separately by test_bodies_host.py::test_tree_structure -- and computes every triangle and every box itself."""
import numpy as np

F = np.float32
SUN = (-0.1, -0.05, -1.0)                    # sun_dir as the scene carries it: the renderer NEGATES it (src/gpu_render.cu:802-806), so light comes ...
TO_SUN = (0.1, 0.05, 1.0)                    # ... from here: nearly straight above body 0's panel, no zero component
LOOKFROM, LOOKAT, VFOV = (0.0, -14.0, 16.0), (0.0, 0.0, 0.0), 40.0
PATCH_HALF = 1.5                             # body 2's square patch is [-1.5, 1.5]^2 around its origin ...
PATCH_AT = (2.0, 1.0, 3.0)                   # ... and P3 puts that origin here, above the panel
PATCH_REST = (-10.0, 8.0, 2.0)


def _tris(v, n=None, mat=0):
    """TRI_DTYPE-shaped dict arrays from (k, 3, 3) vertices; face normals unless given."""
    v = np.asarray(v, F).reshape(-1, 3, 3)
    if n is None:
        fn = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
        fn = (fn / np.linalg.norm(fn, axis=1, keepdims=True)).astype(F)
        n = np.repeat(fn[:, None, :], 3, axis=1)
    return v, np.asarray(n, F).reshape(-1, 3, 3), np.full(len(v), mat, np.int32)


def _grid(origin, du, dv, nu, nv):
    """nu x nv quads (two triangles each) spanned by du, dv from origin."""
    o, du, dv = (np.asarray(a, np.float64) for a in (origin, du, dv))
    out = []
    for i in range(nu):
        for j in range(nv):
            a, b, c, d = o + i * du + j * dv, o + (i + 1) * du + j * dv, o + (i + 1) * du + (j + 1) * dv, o + i * du + (j + 1) * dv
            out += [(a, b, c), (a, c, d)]
    return np.array(out)


def body_triangles():
    """[(v, n, material)] per body -- under 600 triangles in all."""
    # body 0: a 12 x 12 panel in z = 0 (288 triangles; every leaf box is flat: the pad case of the static part) and a strip whose normals are not face normals
    panel = _grid((-6, -6, 0), (1, 0, 0), (0, 1, 0), 12, 12)
    strip = _grid((-6, -5.75, 0.5), (1, 0, 0.03), (0, 0.5, 0.02), 3, 1)
    tilt = np.array([0.3, 0.1, 1.0]) / np.linalg.norm([0.3, 0.1, 1.0])
    strip_n = np.tile(np.array([tilt, [0.0, 0.0, 1.0], [-0.2, 0.25, 0.94]]), (len(strip), 1, 1))
    v0, n0, m0 = _tris(panel)
    v0s, n0s, m0s = _tris(strip, strip_n, 1)
    # body 1: a closed box, 4 x 4 quads per face (192 triangles), and an axis-aligned flat panel well away from it (flat in x at rest: the pad case of a movable body)
    c, h = np.array([8.0, 0.0, 3.0]), 1.0
    faces = []
    for ax in range(3):
        u, w = np.eye(3)[(ax + 1) % 3], np.eye(3)[(ax + 2) % 3]
        for s in (-1.0, 1.0):
            o = c + s * h * np.eye(3)[ax] - h * u - h * w
            du, dv = (u, w) if s > 0 else (w, u)                   # outward winding
            faces.append(_grid(o, du * (2 * h / 4), dv * (2 * h / 4), 4, 4))
    flat = _grid((11.5, -1.0, 2.0), (0, 0.5, 0), (0, 0, 0.5), 4, 2)
    v1, n1, m1 = _tris(np.concatenate(faces + [flat]), mat=1)
    # body 2: three triangles, a single leaf: a square patch (two triangles) and a flap just above it
    p = PATCH_HALF
    o = np.array(PATCH_REST)
    A, B, C_, D = o + (-p, -p, 0), o + (p, -p, 0), o + (p, p, 0), o + (-p, p, 0)
    up = np.array([0.0, 0.0, 0.2])
    v2, n2, m2 = _tris(np.array([(A, B, C_), (A, C_, D), (A + up, B + up, D + up)]))
    # body 3: nine triangles with one common centroid, exactly (c + a, c + b, c - a - b with dyadic a, b): a big leaf
    cc = np.array([-9.0, -8.0, 4.0])
    nine = []
    for k in range(9):
        a = np.array([0.25 * (k + 1), 0.5, 0.25 * (k % 3)])
        b = np.array([-0.5, 0.25 * (k + 2), -0.25 * (k % 2)])
        nine.append((cc + a, cc + b, cc - a - b))
    v3, n3, m3 = _tris(np.array(nine), mat=1)
    return [(np.concatenate([v0, v0s]), np.concatenate([n0, n0s]), np.concatenate([m0, m0s])), (v1, n1, m1), (v2, n2, m2), (v3, n3, m3)]


def build_scene(dsrt):
    """HostScene with the four bodies and the bodies tree, at rest."""
    from dsrt_amd import capi
    mats = np.zeros(2, capi.MAT_DTYPE)
    mats["albedo_tex"] = -1
    mats["albedo"] = [(0.7, 0.7, 0.7), (0.8, 0.5, 0.3)]
    mats["ref_idx"] = 1.5
    hs = dsrt.HostScene()
    for b, (v, n, m) in enumerate(body_triangles()):
        if b:
            assert hs.begin_body() == b
        t = np.zeros(len(v), capi.TRI_DTYPE)
        t["v"], t["n"], t["material_id"], t["albedo_tex"] = v, n, m, -1
        hs.add_arrays(tris=t, mats=mats)              # (add_arrays rebases the ids onto the scene's table: every body brings its two materials)
    hs.build_bvh_bodies()
    return hs


def _rot(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def _pose(R, t):
    return np.concatenate([np.asarray(R, np.float64), np.asarray(t, np.float64).reshape(3, 1)], axis=1).astype(F).reshape(12)


def pose_sets():
    """{name: (3, 12) float32} for bodies 1, 2, 3."""
    I = np.eye(3)
    P1 = np.stack([_pose(I, (0, 0, 0))] * 3)
    P2 = np.stack([_pose(_rot((1, 2, 3), np.sqrt(2.0)), (-3.0, 2.5, 1.25)),
                   _pose(_rot((-2, 1, 0.5), np.pi / np.e), (4.0, -6.0, 0.75)),
                   _pose(_rot((0.3, -1, 2), np.sqrt(7.0)), (5.5, 3.0, -2.0))])
    Rz90 = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])                    # exact: body 1's panel, flat in x at rest, is flat in y afterwards
    P3 = np.stack([_pose(Rz90, (0, 0, 0)),
                   _pose(I, np.array(PATCH_AT) - np.array(PATCH_REST)),                       # body 2 between the Sun and body 0's panel
                   _pose(_rot((1, 1, 0), 1.0), (0.5, 0.25, 0.0))])
    return {"P1": P1, "P2": P2, "P3": P3}


# ---- the model ----------------------------------------------------------------------------------------------------------------------------------------------

def pose_points(pose, v):
    r = np.asarray(pose, F).reshape(3, 4)
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    return np.stack([((r[i, 0] * x + r[i, 1] * y) + r[i, 2] * z) + r[i, 3] for i in range(3)], axis=-1).astype(F)


def pose_dirs(pose, v):
    r = np.asarray(pose, F).reshape(3, 4)
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    return np.stack([(r[i, 0] * x + r[i, 1] * y) + r[i, 2] * z for i in range(3)], axis=-1).astype(F)


def body_pad(rest_v):
    """flat_box_pad(largest edge of the body's unpadded rest-pose root box)."""
    p = rest_v.reshape(-1, 3)
    ext = F((p.max(axis=0) - p.min(axis=0)).astype(F).max())
    return F(ext * F(1.0 / 4096.0)) if ext > 0 else F(1.0e-6)


def chain_and_roots(nodes, ranges):
    """(chain nodes T0.., {body: root node}) of the bodies tree with the body ranges [(first, count)]."""
    live = [b for b, (_, n) in enumerate(ranges) if n > 0]
    chain, roots, t = [], {}, 0
    for b in live[:-1]:
        chain.append(t)
        roots[b] = int(nodes[t]["left"])
        t = int(nodes[t]["right"])
    if live:
        roots[live[-1]] = t
    return chain, roots


def subtree(nodes, root):
    out, todo = [], [root]
    while todo:
        n = todo.pop()
        out.append(n)
        if nodes[n]["tri_count"] == 0:
            todo += [int(nodes[n]["right"]), int(nodes[n]["left"])]
    return out


def model_update(rest_tris, nodes, idx, ranges, poses):
    """(v, n, bbox_min, bbox_max) of the scene with `poses` {body: 12 floats} applied to the REST triangles; bodies not named keep their rest triangles."""
    v, n = rest_tris["v"].astype(F).copy(), rest_tris["n"].astype(F).copy()
    for b, p in poses.items():
        first, cnt = ranges[b]
        v[first:first + cnt] = pose_points(p, rest_tris["v"][first:first + cnt])
        n[first:first + cnt] = pose_dirs(p, rest_tris["n"][first:first + cnt])
    lo, hi = np.zeros((len(nodes), 3), F), np.zeros((len(nodes), 3), F)
    chain, roots = chain_and_roots(nodes, ranges)
    for b, root in roots.items():
        first, cnt = ranges[b]
        pad = body_pad(rest_tris["v"][first:first + cnt])
        for k in sorted(subtree(nodes, root), reverse=True):                                  # pre-order numbering: children after their parent
            nd = nodes[k]
            if nd["tri_count"] > 0:
                pts = v[idx[nd["tri_offset"]:nd["tri_offset"] + nd["tri_count"]]].reshape(-1, 3)
                l, h = pts.min(axis=0) + F(0.0), pts.max(axis=0) + F(0.0)                      # canonical zero
                flat = h == l
                lo[k], hi[k] = np.where(flat, l - pad, l), np.where(flat, h + pad, h)
            else:
                lo[k], hi[k] = np.minimum(lo[nd["left"]], lo[nd["right"]]), np.maximum(hi[nd["left"]], hi[nd["right"]])
    for k in reversed(chain):
        nd = nodes[k]
        lo[k], hi[k] = np.minimum(lo[nd["left"]], lo[nd["right"]]), np.maximum(hi[nd["left"]], hi[nd["right"]])
    return v, n, lo, hi
