"""Synthetic triangle sets [N, 3 vertices, 3 axes] float32 for the LBVH tests (tests/test_oracle_lbvh.py, tests/test_gpu_lbvh.py)."""
import numpy as np

F = np.float32
SIZES = (1, 2, 3, 4, 5, 6, 8, 9, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000)


def random_tris(n, seed, size=0.3):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-5.0, 7.0, (n, 1, 3))
    return (c + rng.normal(scale=size, size=(n, 3, 3))).astype(F)


def quad(z=0.0, h=1.0, axis=2):
    """Two triangles of a square in the plane coordinate[axis] = z (flat on that axis: the whole scene has zero thickness there)."""
    p = np.array([[-h, -h, z], [h, -h, z], [h, h, z], [-h, h, z]], F)
    p = np.roll(p, axis - 2, axis=1)
    return np.stack([p[[0, 1, 2]], p[[0, 2, 3]]]).astype(F)


def panel(n, y=0.5):
    """n triangles in the plane y = const, side by side along x."""
    t = np.zeros((n, 3, 3), F)
    for i in range(n):
        t[i] = [[i, y, 0.0], [i + 1.0, y, 0.0], [i + 0.5, y, 1.0]]
    return t


def flat_and_solid(n, seed):
    """Flat triangles on each axis between non-flat ones."""
    t = random_tris(n, seed)
    for i in range(0, n, 3):
        t[i, :, i % 3] = t[i, 0, i % 3]
    return t


def copies(n):
    return np.repeat(np.array([[[0.1, 0.2, 0.3], [1.1, 0.4, 0.2], [0.5, 1.3, 0.9]]], F), n, axis=0)


def rotated(n):
    """n triangles turned about one common centre, plus two far points that set the scene's extent: (almost) all codes equal."""
    th = np.linspace(0.0, 2.0 * np.pi, n, endpoint=False)[:, None] + np.array([0.0, 2.0 * np.pi / 3.0, 4.0 * np.pi / 3.0])
    t = np.stack([np.cos(th), np.sin(th), 0.3 * np.cos(2.0 * th)], axis=2) * 1e-3 + np.array([1.0, 2.0, 3.0])
    far = np.array([[[-100.0] * 3] * 3, [[100.0] * 3] * 3])
    return np.concatenate([t, far]).astype(F)


def one_point(n, p=(1.5, -2.0, 0.25)):
    return np.tile(np.array(p, F), (n, 3, 1)).astype(F)


def line(n, axis=0):
    """Triangles along one axis, the same in the other two: codes that differ in one axis only."""
    t = np.zeros((n, 3, 3), F)
    base = np.array([[0.0, 0.0, 0.0], [0.5, 0.2, 0.0], [0.2, 0.0, 0.3]], F)
    base = np.roll(base, axis, axis=1)
    for i in range(n):
        t[i] = base
        t[i, :, axis] += F(i)
    return t


def signed_zeros(n, seed):
    """Box faces at zero whose vertices hold -0.0 and +0.0 in every order, on both sides of the origin."""
    rng = np.random.default_rng(seed)
    t = random_tris(n, seed, size=1.0)
    for i in range(n):
        a = i % 3
        t[i, :, a] = np.abs(t[i, :, a]) * (1 if i % 2 else -1)
        zs = [F(-0.0), F(0.0)]
        j = rng.permutation(3)
        t[i, j[0], a], t[i, j[1], a] = zs[rng.integers(0, 2)], zs[rng.integers(0, 2)]
    return t.astype(F)


def small_signed_zeros():
    """Two triangles whose boxes start at -0.0 and +0.0 on x (a single leaf)."""
    return np.array([[[-0.0, 0.0, 0.0], [1.0, 1.0, 0.0], [0.0, 1.0, 1.0]],
                     [[0.0, 2.0, 0.0], [1.0, 3.0, 0.5], [-0.0, 2.5, 1.0]]], F)


def huge(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.uniform(1.0e30, 3.0e30, (n, 1, 3)) * np.array([1.0, -1.0, 1.0]) + rng.normal(scale=1e28, size=(n, 3, 3))).astype(F)


def ulp_cluster(n, seed):
    """Non-flat triangles a few ulps wide around (1, 2, 3): the scene is a few ulps wide as well."""
    rng = np.random.default_rng(seed)
    base = np.array([1.0, 2.0, 3.0], F)
    steps = rng.integers(0, 6, (n, 1, 3)) + np.array([[0, 0, 0], [1, 2, 0], [2, 0, 1]])
    out = np.empty((n, 3, 3), F)
    for a in range(3):
        x = np.full(steps[..., a].shape, base[a], F)
        for k in range(int(steps[..., a].max())):
            x = np.where(steps[..., a] > k, np.nextafter(x, F(np.inf)), x)
        out[..., a] = x
    return out


def top_end(n, seed):
    """Points at the scene's upper corner (u = 1, clamped) and up to two 2^-22 of the extent below it, between random triangles."""
    rng = np.random.default_rng(seed)
    t = rng.uniform(0.0, 1.0, (n, 3, 3)).astype(F)
    k = n // 4
    pts = np.ones((k, 3), F) - (rng.integers(0, 3, (k, 3)) * F(2.0 ** -22)).astype(F)
    pts[0] = 1.0
    t[:k] = pts[:, None, :]
    t[k, :, :] = 0.0
    return t


def clamp_edge(extra, seed):
    """Centroids on both sides of the clamp at 2^21 - 1 in a [0, 1]^3 scene: x = 1 (clamped) and x = 1 - 3 * 2^-22 (2^21 - 2), the latter
    once with z in the first quantum above 0, in an input order that a different clamp would change; then `extra` random triangles."""
    xb, z1 = 1.0 - 3.0 * 2.0 ** -22, 1.5 * 2.0 ** -21
    pts = np.array([[xb, 0.0, 0.0], [xb, 0.0, z1], [1.0, 0.0, 0.0], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]], F)
    t = np.repeat(pts[:, None, :], 3, axis=1)
    return np.concatenate([t, np.random.default_rng(seed).uniform(0.1, 0.9, (extra, 3, 3)).astype(F)]).astype(F)


def nested(bits, tail):
    """Point triangles whose codes nest: one per code bit from the top (coordinate 2^-(1 + j // 3) on axis j % 3), `tail` points at the
    origin (equal codes) and one at (1, 1, 1), which fixes the scene box to [0, 1]^3.  A chain as deep as `bits`, then a balanced tail."""
    pts = [np.ones(3)]
    for j in range(bits):
        p = np.zeros(3)
        p[j % 3] = 2.0 ** -(1 + j // 3)
        pts.append(p)
    pts += [np.zeros(3)] * tail
    return np.repeat(np.array(pts, F)[:, None, :], 3, axis=1)


def synthetic_cases():
    """name -> triangles, for every case both test files run."""
    cases = {f"random_{n}": random_tris(n, n) for n in SIZES}
    cases.update({f"quad_axis{a}": quad(0.25, 1.0, a) for a in range(3)})
    cases.update({f"panel_{n}": panel(n) for n in range(1, 9)})
    cases["one_flat_triangle"] = panel(1)
    cases.update({f"flat_and_solid_{n}": flat_and_solid(n, 3) for n in (4, 9, 200)})
    cases["copies_1000"] = copies(1000)
    cases["copies_3"] = copies(3)
    cases["rotated_300"] = rotated(300)
    cases.update({f"one_point_{n}": one_point(n) for n in (1, 3, 7, 100)})
    cases.update({f"line_axis{a}": line(100, a) for a in range(3)})
    cases["signed_zeros_300"] = signed_zeros(300, 1)
    cases["signed_zeros_small"] = small_signed_zeros()
    cases["huge_500"] = huge(500, 2)
    cases["ulp_cluster_300"] = ulp_cluster(300, 4)
    cases["top_end_400"] = top_end(400, 5)
    cases["clamp_edge_200"] = clamp_edge(195, 6)
    for bits, tail in ((20, 40), (55, 3), (60, 16), (62, 1), (63, 0), (63, 64), (63, 300)):
        cases[f"nested_{bits}_{tail}"] = nested(bits, tail)
    return cases


def tri_records(verts, capi):
    """TRI_DTYPE records for add_arrays (material 0, no texture, normals from the winding)."""
    t = np.zeros(len(verts), capi.TRI_DTYPE)
    t["v"] = verts
    v = verts.astype(np.float64)
    nrm = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    ln = np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm = np.where(ln > 0, nrm / np.where(ln > 0, ln, 1.0), np.array([0.0, 0.0, 1.0]))
    t["n"] = np.repeat(nrm[:, None, :], 3, axis=1).astype(F)
    t["material_id"] = 0
    t["albedo_tex"] = -1
    return t


def one_material(capi):
    m = np.zeros(1, capi.MAT_DTYPE)
    m["type"] = 0
    m["albedo_tex"] = -1
    m["albedo"] = [0.7, 0.6, 0.5]
    return m
