"""The CPU model of the motion stage (include/dsrt.h, TEMPORAL ACCUMULATION WITH BODIES) on top of tests/_temporal_model.py and tests/_bodies_model.py: which body
a pixel lies on, which bodies moved, and where a moved body's surface point and normal were in the previous frame -- numpy float32, every step one correctly
rounded IEEE operation in the header's order.  The temporal stage itself is _temporal_model.stage, fed (N', X') for the terms that face the history.  Shared by
tests/test_temporal_bodies_host.py (CPU) and tests/test_gpu_temporal_bodies.py, which holds the kernel to it bit for bit."""
import numpy as np

from _bodies_model import pose_dirs, pose_points
from _denoise_model import F, FLT_MAX, filterable, iterate, start
from _temporal_model import DEFAULTS, pack_history, stage


def body_of(prim_id, first_tri, num_tris):
    """b(p): the body >= 1 whose triangle range holds prim_id, otherwise 0 (body 0's triangles, spheres, misses, anything else)."""
    prim = np.asarray(prim_id, np.int64)
    body = np.zeros(prim.shape, np.int64)
    for b in range(1, len(first_tri)):
        body[(prim >= int(first_tri[b])) & (prim < int(first_tri[b]) + int(num_tris[b]))] = b
    return body


def moved_bodies(poses_prev, poses_cur):
    """[bodies] bool: any of the 12 pose floats differs (!=); body 0 never moves."""
    pp, pc = (np.asarray(p, F).reshape(-1, 12) for p in (poses_prev, poses_cur))
    moved = (pp != pc).any(axis=1)
    moved[0] = False
    return moved


def _transposed(pose):
    """The pose whose rotation is the transpose of `pose`'s, without a translation: pose_dirs of it is the header's transpose product."""
    r = np.asarray(pose, F).reshape(3, 4)
    t = np.zeros((3, 4), F)
    t[:, :3] = r[:, :3].T
    return t


def motion(first_tri, num_tris, poses_prev, poses_cur, prim_id, normal, position):
    """(N', X') of N_p, X_p (..., 3) and prim_id (...)."""
    N, X = np.asarray(normal, F), np.asarray(position, F)
    pp, pc = (np.asarray(p, F).reshape(-1, 12) for p in (poses_prev, poses_cur))
    body = body_of(prim_id, first_tri, num_tris)
    moved = moved_bodies(pp, pc)
    N2, X2 = N.copy(), X.copy()
    with np.errstate(all="ignore"):
        for b in np.nonzero(moved)[0]:
            on = body == b
            if not on.any():
                continue
            c, q = pc[b].reshape(3, 4), pp[b]
            d = (X[on] - c[:, 3]).astype(F)
            X2[on] = pose_points(q, pose_dirs(_transposed(c), d))
            N2[on] = pose_dirs(q, pose_dirs(_transposed(c), N[on]))
    return N2, X2


def denoise_temporal_bodies(S, S2, n, guides, mo, prev_cam=None, prev=None, temporal=None, iterations=5, normal_power_log2=5, sigma_l=1.0, sigma_z=0.01, sigma_a=0.1):
    """One frame with the motion stage; mo = (first_tri, num_tris, poses_prev, poses_cur, prim_id (H, W)).  _temporal_model.denoise_temporal's dict and
    "prev_position" (X' where range <= FLT_MAX, +0 elsewhere), "prev_normal"."""
    c, v = start(S, S2, n)
    Fm = filterable(guides["range"], n)
    N, X = np.asarray(guides["normal"], F), np.asarray(guides["position"], F)
    N2, X2 = motion(*mo[:4], np.asarray(mo[4]).reshape(Fm.shape), N, X)
    facing = {**guides, "normal": N2, "position": X2}                          # what meets the previous frame: the projection, both tap tests, the guard
    cb, vb, m, prev_xy, found = stage(c, v, n, Fm, facing, prev_cam, prev, **(temporal or DEFAULTS))
    nxt = pack_history(cb, m, vb, N, X)                                         # the record keeps the current N_p, X_p
    c, v = cb, vb
    for i in range(iterations):
        c, v = iterate(c, v, Fm, guides, 1 << i, normal_power_log2, sigma_l, sigma_z, sigma_a)
    with np.errstate(invalid="ignore"):
        hit = np.asarray(guides["range"], F) <= FLT_MAX
    return {"linear": c, "var": v, "next": nxt, "prev_xy": prev_xy, "weight": m, "found": found, "blended": (cb, vb),
            "prev_position": np.where(hit[..., None], X2, F(0)).astype(F), "prev_normal": N2}
