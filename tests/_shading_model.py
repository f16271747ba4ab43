"""The CPU model of the temporal stage that follows shading (include/dsrt.h, TEMPORAL ACCUMULATION THAT FOLLOWS SHADING) on top of tests/_temporal_model.py and
tests/_motion_model.py: the bodies stage with every record's sun state in word 15, the tap test on it, the two shadow-edge guards and the status byte -- numpy
float32 on whole-image arrays, the taps in the header's order, every step one correctly rounded IEEE operation.  A skipped tap leaves every sum as it is.  Shared
by tests/test_temporal_shading_host.py (CPU) and tests/test_gpu_temporal_shading.py, which holds the kernel to it bit for bit."""
import numpy as np

from _denoise_model import F, FLT_MAX, dot, filterable, iterate, start
from _motion_model import motion
from _temporal_model import DEFAULTS, QNAN, pack_history, project

HIT, SUN = 1, 8                                                               # DSRT_GB_HIT, DSRT_GB_SUN_VISIBLE
PROJECTED, FOUND, FOUND_GEOMETRY, EDGE_PREV, EDGE_CUR = 1, 2, 4, 8, 16        # the status byte's bits
INFO = {}


def sun_state(flags, rng):
    """s_p: 2 lit, 1 in shadow, +0 where the pixel is a miss (!(range <= FLT_MAX))."""
    with np.errstate(invalid="ignore"):
        hit = np.asarray(rng, F) <= FLT_MAX
    return np.where(hit, np.where((np.asarray(flags, np.uint8) & SUN) != 0, F(2), F(1)), F(0)).astype(F)


def mismatch(sq, sp):
    """mis(q) = !(s_q == 0 || s_q == s_p): NaN and any stray value mismatch, -0 is unknown like +0."""
    with np.errstate(invalid="ignore"):
        return ~((sq == F(0)) | (sq == sp))


def edge_cur(flags):
    """Over the 3 x 3 block around p inside the image: any neighbour r with (flags_r & 1) and (flags_r & 8) != (flags_p & 8)."""
    f = np.asarray(flags, np.uint8)
    H, W = f.shape
    out = np.zeros((H, W), bool)
    ys, xs = np.mgrid[0:H, 0:W]
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            qy, qx = ys + dy, xs + dx
            inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
            fr = f[np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)]
            out |= inside & ((fr & HIT) != 0) & ((fr & SUN) != (f & SUN))
    return out


def stage(c, v, n, Fm, guides, flags, edge_guard, prev_cam, prev, alpha_min=0.1, normal_cos_min=0.9, plane_tol=0.01, min_support=0.9):
    """(c', v', m', prev_xy, found, status) -- _temporal_model.stage with the sun state: `guides` are what faces the history (N', X', and the current range), flags
    the current frame's, prev = float32 (H, W, 16) with the records' states in word 15, or None.  INFO holds the last call's masks."""
    N, X, rng = (np.asarray(guides[k], F) for k in ("normal", "position", "range"))
    flags = np.asarray(flags, np.uint8)
    H, W = Fm.shape
    nf = np.broadcast_to(np.asarray(n, np.uint32), (H, W)).astype(F)
    prev_xy = np.full((H, W, 2), QNAN, F)
    found = np.zeros((H, W), bool)
    status = np.zeros((H, W), np.uint8)
    m_out = np.where(Fm, nf, F(0)).astype(F)
    c_out, v_out = c.copy(), v.copy()
    if prev is None:
        return c_out, v_out, m_out, prev_xy, found, status
    prev = np.asarray(prev, F).reshape(H, W, 16)
    sp = sun_state(flags, rng)
    with np.errstate(all="ignore"):
        fx, fy, ok = project(X, prev_cam, W, H)
        projected = ok & (rng <= FLT_MAX)
        prev_xy[..., 0] = np.where(projected, fx, QNAN)
        prev_xy[..., 1] = np.where(projected, fy, QNAN)
        use = projected & Fm
        fxs, fys = np.where(use, fx, F(0)), np.where(use, fy, F(0))          # (indices are formed for the pixels that tap only)
        flx, fly = np.floor(fxs), np.floor(fys)
        x0, y0 = flx.astype(np.int64), fly.astype(np.int64)
        wx, wy = fxs - flx, fys - fly
        ox, oy = F(1) - wx, F(1) - wy
        tol = F(plane_tol) * rng
        sw, sm, swg = np.zeros((H, W), F), np.zeros((H, W), F), np.zeros((H, W), F)
        sc, sv = np.zeros((H, W, 3), F), np.zeros((H, W, 3), F)
        seen, seen_g = np.zeros((H, W), bool), np.zeros((H, W), bool)
        tap_mis = np.zeros((H, W), bool)
        for dx, dy, b in ((0, 0, ox * oy), (1, 0, wx * oy), (0, 1, ox * wy), (1, 1, wx * wy)):
            qx, qy = x0 + dx, y0 + dy
            inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            rec = prev[np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)]
            cq, mq, vq, Nq, Xq, sq = rec[..., 0:3], rec[..., 3], rec[..., 4:7], rec[..., 8:11], rec[..., 12:15], rec[..., 15]
            geo = use & inside & (mq > 0) & (dot(N, Nq) >= F(normal_cos_min)) & (np.abs(dot(N, Xq - X)) <= tol)
            seen_g |= geo & (b >= F(0.99))
            swg = np.where(geo, swg + b, swg)
            take = geo & ~mismatch(sq, sp)
            tap_mis |= geo & ~take
            seen |= take & (b >= F(0.99))
            sw = np.where(take, sw + b, sw)
            sc = np.where(take[..., None], sc + b[..., None] * cq, sc)
            sv = np.where(take[..., None], sv + b[..., None] * vq, sv)
            sm = np.where(take, sm + b * mq, sm)
        guarded, e_prev = np.zeros((H, W), bool), np.zeros((H, W), bool)          # the occluder guard's 4 x 4 block: the guard, and the previous frame's edge
        for gy in range(-1, 3):
            for gx in range(-1, 3):
                qx, qy = x0 + gx, y0 + gy
                inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                rec = prev[np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)]
                usable = use & inside & (rec[..., 3] > 0)
                guarded |= usable & (dot(N, rec[..., 12:15] - X) > tol)
                e_prev |= usable & mismatch(rec[..., 15], sp)
        e_cur = use & edge_cur(flags)
        found_geometry = use & (swg >= F(min_support)) & (seen_g | ~guarded)
        taps_found = use & (sw >= F(min_support)) & (seen | ~guarded)
        found = taps_found & ~(bool(edge_guard) & (e_prev | e_cur))
        status = (projected * PROJECTED + found * FOUND + found_geometry * FOUND_GEOMETRY + e_prev * EDGE_PREV + e_cur * EDGE_CUR).astype(np.uint8)
        INFO.update(guarded=guarded, seen=seen, use=use, tap_mis=tap_mis, taps_found=taps_found, edge_prev=e_prev, edge_cur=e_cur, found_geometry=found_geometry)
        ch, vh, mh = sc / sw[..., None], sv / sw[..., None], sm / sw
        alpha = np.fmax(nf / (nf + mh), F(alpha_min))
        beta = F(1) - alpha
        cb = beta[..., None] * ch + alpha[..., None] * c
        vb = (beta * beta)[..., None] * vh + (alpha * alpha)[..., None] * v
        c_out = np.where(found[..., None], cb, c).astype(F)
        v_out = np.where(found[..., None], vb, v).astype(F)
        m_out = np.where(found, nf / alpha, m_out).astype(F)
    return c_out, v_out, m_out, prev_xy, found, status


def denoise_temporal_shaded(S, S2, n, guides, flags, mo=None, edge_guard=1, prev_cam=None, prev=None, temporal=None, iterations=5, normal_power_log2=5, sigma_l=1.0,
                            sigma_z=0.01, sigma_a=0.1):
    """One frame; mo = (first_tri, num_tris, poses_prev, poses_cur, prim_id (H, W)) or None for a static scene.  _motion_model.denoise_temporal_bodies' dict --
    "prev_position" is None without a motion -- plus "status" (uint8 (H, W)); word 15 of "next" is the sun state."""
    c, v = start(S, S2, n)
    Fm = filterable(guides["range"], n)
    N, X = np.asarray(guides["normal"], F), np.asarray(guides["position"], F)
    flags = np.asarray(flags, np.uint8).reshape(Fm.shape)
    N2, X2 = motion(*mo[:4], np.asarray(mo[4]).reshape(Fm.shape), N, X) if mo is not None else (N, X)
    facing = {**guides, "normal": N2, "position": X2}                          # what meets the previous frame: the projection, both tap tests, the guard
    cb, vb, m, prev_xy, found, status = stage(c, v, n, Fm, facing, flags, edge_guard, prev_cam, prev, **(temporal or DEFAULTS))
    nxt = pack_history(cb, m, vb, N, X)                                         # the record keeps the current N_p, X_p ...
    nxt[..., 15] = sun_state(flags, guides["range"])                            # ... and the current sun state
    c, v = cb, vb
    for i in range(iterations):
        c, v = iterate(c, v, Fm, guides, 1 << i, normal_power_log2, sigma_l, sigma_z, sigma_a)
    with np.errstate(invalid="ignore"):
        hit = np.asarray(guides["range"], F) <= FLT_MAX
    return {"linear": c, "var": v, "next": nxt, "prev_xy": prev_xy, "weight": m, "found": found, "blended": (cb, vb), "status": status,
            "prev_position": np.where(hit[..., None], X2, F(0)).astype(F) if mo is not None else None, "prev_normal": N2}


# ---- frames for the tests ----
STRAY_STATES = np.array([0x00000000, 0x80000000, 0x7FC00000, 0x40400000], np.uint32).view(F)          # +0, -0, NaN, 3


def shadow_flags(rng, rng_img, edges, shift=0.0):
    """A flags image for the guides' `range` image: DSRT_GB_HIT where the range is finite, the front-face and sphere bits at random, and the sun bit in stripes
    between straight edges (nx, ny, d): lit flips across nx*x + ny*y = d + shift.  Misses keep a random sun bit: their state is 0 whatever it says."""
    H, W = rng_img.shape
    ys, xs = np.mgrid[0:H, 0:W]
    lit = np.ones((H, W), bool)
    for nx, ny, d in edges:
        lit ^= (nx * xs + ny * ys) > d + shift
    with np.errstate(invalid="ignore"):
        hit = np.asarray(rng_img, F) <= FLT_MAX
    lit = np.where(hit, lit, rng.random((H, W)) < 0.5)
    return (hit * HIT | rng.integers(0, 4, (H, W)) * 2 * hit | lit * SUN).astype(np.uint8)


def with_states(rng, history, flags, stray=0.0):
    """`history` with word 15 set to the sun state `flags` shows (2 lit, 1 otherwise), a fraction `stray` of the records given one of STRAY_STATES instead."""
    h = np.array(history, F)
    s = np.where((np.asarray(flags, np.uint8) & SUN) != 0, F(2), F(1)).astype(F)
    odd = rng.random(s.shape) < stray
    s[odd] = STRAY_STATES[rng.integers(0, len(STRAY_STATES), int(odd.sum()))]
    h[..., 15] = s
    return h


# Shadow edges per image size for shadow_flags, and the shift of the history's edges against them: chosen on the CPU so that every status class below holds at least
# a sixteenth of the image (tests/test_temporal_shading_host.py prints the counts).
EDGES = {(33, 17): ((1.0, 0.25, 9.0), (1.0, -0.2, 22.0)), (37, 29): ((1.0, 0.3, 10.0), (0.2, 1.0, 17.0), (1.0, -0.25, 27.0)),
         (64, 48): ((1.0, 0.3, 14.0), (0.2, 1.0, 20.0), (1.0, -0.25, 45.0))}
EDGE_SHIFT = 2.5


def status_classes(on, off, present_found):
    """What became of the pixels' history, from the status bytes of the stage with edge_guard 1 (`on`) and 0 (`off`) and the present stage's decision: the pixels
    that keep it, that lose it to the tap test, and that lose it with edge_prev / edge_cur set (a pixel may be lost to several causes at once); "only edge_prev" /
    "only edge_cur": the taps alone would have found history and the one guard voids it."""
    bit = lambda r, b: (r["status"] & b) != 0                                        # noqa: E731
    lost = bit(on, FOUND_GEOMETRY) & ~bit(on, FOUND)
    return {"keep": bit(on, FOUND), "tap test": present_found & ~bit(off, FOUND), "edge_prev": lost & bit(on, EDGE_PREV), "edge_cur": lost & bit(on, EDGE_CUR),
            "only edge_prev": bit(off, FOUND) & bit(off, EDGE_PREV) & ~bit(off, EDGE_CUR), "only edge_cur": bit(off, FOUND) & bit(off, EDGE_CUR) & ~bit(off, EDGE_PREV)}
