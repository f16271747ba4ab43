"""The CPU model of the coverage pass and of coverage demodulation (include/dsrt.h, COVERAGE and DENOISER: COVERAGE DEMODULATION).

Coverage: per sub-sample the G-buffer record the oracle's exported functions define -- dsrt_oracle_camera_ray(cam, x, H-1-r, W, H, jx, jy), dsrt_oracle_scene_hit,
the derived channels in numpy float32 operation by operation and the shadow ray through dsrt_oracle_scene_hit again, exactly as tests/test_gpu_gbuffer.py's
expected_gbuffer builds the centre ray's -- then the header's reduction: counts, masks, class counts and the representative.  Demodulation: tests/_denoise_model.py's
iterations between the header's division and multiplication.  Shared by tests/test_coverage_host.py (CPU) and tests/test_gpu_coverage.py (bit for bit)."""
import ctypes as C

import numpy as np

from _denoise_model import F, filterable, iterate, start

GRID, DIAGONAL = 0, 1
GB_KEYS = ("t", "range", "depth", "position", "normal", "uv", "albedo", "prim_id", "material_id", "sun_cos", "flags")


def legal():
    """Every legal (pattern, samples)."""
    return [(GRID, s) for s in range(1, 9)] + [(DIAGONAL, n) for n in range(1, 65)]


def count(pattern, samples):
    return samples * samples if pattern == GRID else samples


def offsets(pattern, samples):
    """(jx, jy, key) of sub-samples k = 0 .. n-1: float32, float32, int -- the header's arithmetic, one correctly rounded operation per step."""
    n = count(pattern, samples)
    k = np.arange(n)
    if pattern == GRID:
        assert 1 <= samples <= 8
        i, j = k % samples, k // samples
        jx = (i.astype(F) + F(0.5)) / F(samples)
        jy = (j.astype(F) + F(0.5)) / F(samples)
        key = (2 * i + 1 - samples) ** 2 + (2 * j + 1 - samples) ** 2
    else:
        assert pattern == DIAGONAL and 1 <= samples <= 64
        jx = jy = (k.astype(F) + F(0.5)) / F(n)
        key = (2 * k + 1 - n) ** 2
    return jx.astype(F), jy.astype(F), key


def rep_order(pattern, samples):
    """The sub-samples in the order the representative prefers them: smallest key first, ties to the smaller k."""
    _, _, key = offsets(pattern, samples)
    return np.lexsort((np.arange(key.size), key))


def subsample_gbuffer(oracle, hs, scene, W, H, jx, jy, want_sun=True, want_albedo=True):
    """expected_gbuffer (tests/test_gpu_gbuffer.py) with the pixel offset (jx, jy) in place of (0.5, 0.5): {channel: (H, W[, C])}."""
    from test_gpu_gbuffer import _dot, _oracle_lib, _sphere_roots, _tex2d
    L = _oracle_lib(oracle)
    arrs = hs.arrays()
    n = H * W
    o3, d3 = (C.c_float * 3)(), (C.c_float * 3)()
    out, ids = (C.c_float * 9)(), (C.c_int * 4)()
    O, D = np.zeros((n, 3), F), np.zeros((n, 3), F)
    T, P, N, UV = np.full(n, np.inf, F), np.zeros((n, 3), F), np.zeros((n, 3), F), np.zeros((n, 2), F)
    hit = np.zeros(n, bool)
    IDS = np.full((n, 4), -1, np.int32)
    sp, cam = C.byref(scene), C.byref(scene.camera)
    ray, scene_hit = L.dsrt_oracle_camera_ray, L.dsrt_oracle_scene_hit
    fx, fy = C.c_float(float(jx)), C.c_float(float(jy))
    k = 0
    for r in range(H):
        for x in range(W):
            ray(cam, x, H - 1 - r, W, H, fx, fy, o3, d3)
            O[k], D[k] = o3[:], d3[:]
            if scene_hit(sp, o3, d3, 0.001, 1e9, out, ids):
                hit[k] = True
                T[k], P[k], N[k], UV[k] = out[0], out[1:4], out[4:7], out[7:9]
                IDS[k] = ids[:]
            k += 1
    g = {"t": T}
    with np.errstate(invalid="ignore"):
        g["range"] = np.where(hit, T * np.sqrt(_dot(D, D)), F(np.inf))
        w = scene.camera.w
        neg_w = np.array([-F(w.x), -F(w.y), -F(w.z)], F)
        g["depth"] = np.where(hit, T * _dot(D, np.broadcast_to(neg_w, D.shape)), F(np.inf))
    g["position"], g["normal"], g["uv"] = P, N, UV
    g["material_id"] = np.where(hit, IDS[:, 0], -1).astype(np.int32)
    prim = np.where(hit, IDS[:, 2], -1).astype(np.int32)
    sph_px = np.nonzero(hit & (IDS[:, 2] < 0))[0]
    if sph_px.size:                                                     # sphere s -> -2 - s: the LAST sphere whose root equals the hit's t bit for bit
        found = np.zeros(sph_px.size, bool)
        for s, sph in enumerate(arrs["spheres"]):
            ok, root = _sphere_roots(O[sph_px], D[sph_px], sph)
            same = ok & (root.view(np.uint32) == T[sph_px].view(np.uint32))
            prim[sph_px[same]] = -2 - s
            found |= same
        assert found.all(), "a sphere hit the float32 restatement of hit_sphere does not reproduce"
    g["prim_id"] = prim
    alb = np.zeros((n, 3), F)
    if want_albedo:
        mats, tris = arrs["mats"], arrs["tris"]
        for i in np.nonzero(hit)[0]:
            a = mats[IDS[i, 0]]["albedo"].astype(F)
            if IDS[i, 1] >= 0:
                tri = tris[IDS[i, 2]]
                u, v = UV[i, 0], UV[i, 1]
                wgt = (F(1) - u) - v
                uvs = tri["uv"].astype(F)
                ut = (wgt * uvs[0, 0] + u * uvs[1, 0]) + v * uvs[2, 0]
                vt = (wgt * uvs[0, 1] + u * uvs[1, 1]) + v * uvs[2, 1]
                a = a * _tex2d(arrs, int(IDS[i, 1]), ut, vt)
            alb[i] = a
    g["albedo"] = alb
    cos = np.zeros(n, F)
    visible = np.zeros(n, bool)
    if scene.sun_enabled:
        neg = (C.c_float * 3)(-scene.sun_dir.x, -scene.sun_dir.y, -scene.sun_dir.z)
        l3 = (C.c_float * 3)()
        L.dsrt_oracle_normalize(neg, l3)
        Ld = np.array(l3[:], F)
        cos = np.where(hit, np.maximum(F(0), _dot(N, np.broadcast_to(Ld, N.shape))), F(0)).astype(F)
        if want_sun:
            so = P + N * F(1e-3)
            for i in np.nonzero(hit & (cos > 0))[0]:
                so3 = (C.c_float * 3)(*so[i])
                visible[i] = not scene_hit(sp, so3, l3, 0.001, 1e9, out, ids)
    g["sun_cos"] = cos
    g["flags"] = (hit * 1 | (hit & (IDS[:, 3] == 1)) * 2 | (hit & (IDS[:, 2] < 0)) * 4 | visible * 8).astype(np.uint8)
    return {key: g[key].reshape((H, W) + g[key].shape[1:]) for key in GB_KEYS}


def miss_record(H, W):
    """The G-buffer table's miss values."""
    z = lambda c: np.zeros((H, W, c) if c > 1 else (H, W), F)               # noqa: E731
    return {"t": np.full((H, W), np.inf, F), "range": np.full((H, W), np.inf, F), "depth": np.full((H, W), np.inf, F), "position": z(3), "normal": z(3), "uv": z(2),
            "albedo": z(3), "prim_id": np.full((H, W), -1, np.int32), "material_id": np.full((H, W), -1, np.int32), "sun_cos": z(1), "flags": np.zeros((H, W), np.uint8)}


def in_class(prim, sphere, first, num):
    """prim >= first && (uint32)(prim - first) < (uint32)num; spheres belong to no class."""
    d = (prim.astype(np.int64) - int(first)) & 0xFFFFFFFF
    return ~sphere & (prim >= first) & (d < (int(num) & 0xFFFFFFFF))


def reduce(records, pattern, samples, classes=None):
    """The header's reduction of the n per-sub-sample records (subsample_gbuffer's dicts, k = 0 .. n-1) to the outputs of DsrtCoverage."""
    n = count(pattern, samples)
    assert len(records) == n
    H, W = records[0]["flags"].shape
    hit = [(g["flags"] & 1).astype(bool) for g in records]
    sun = [h & ((g["flags"] & 8) != 0) for h, g in zip(hit, records)]
    out = {}
    for name, bits in (("", hit), ("sun_", sun)):
        cnt = np.zeros((H, W), np.int64)
        mask = np.zeros((H, W), np.uint64)
        for k, b in enumerate(bits):
            cnt += b
            mask |= b.astype(np.uint64) << np.uint64(k)
        out[name + "hits"] = cnt.astype(np.uint8)
        out[name + "alpha"] = (cnt.astype(F) / F(n)).astype(F)
        out[name + "mask"] = mask
    if classes is not None:
        ch = np.zeros((H, W, len(classes)), np.uint8)
        for c, (first, num) in enumerate(classes):
            for h, g in zip(hit, records):
                ch[..., c] += (h & in_class(g["prim_id"], (g["flags"] & 4) != 0, first, num)).astype(np.uint8)
        out["class_hits"] = ch
    rep = miss_record(H, W)
    for k in rep_order(pattern, samples)[::-1]:                         # the most preferred sub-sample is written last
        for key in GB_KEYS:
            m = hit[k] if rep[key].ndim == 2 else hit[k][..., None]
            rep[key] = np.where(m, records[k][key], rep[key])
    out["rep"] = rep
    return out


def coverage(oracle, hs, scene, W, H, pattern, samples, classes=None, want_sun=True, want_albedo=True):
    """The outputs of dsrt_render_coverage for the camera and sun of `scene` (a host view); classes: [(first, num), ...]."""
    jx, jy, _ = offsets(pattern, samples)
    records = [subsample_gbuffer(oracle, hs, scene, W, H, jx[k], jy[k], want_sun, want_albedo) for k in range(jx.size)]
    return reduce(records, pattern, samples, classes)


def coverage_filterable(rng, n, alpha, alpha_min):
    """F_p = (range_p <= FLT_MAX) && n >= 2 && a >= alpha_min; a NaN alpha compares false."""
    with np.errstate(invalid="ignore"):
        return filterable(rng, n) & (np.asarray(alpha, F) >= F(alpha_min))


def denoise_coverage(S, S2, n, guides, alpha, alpha_min, iterations=5, normal_power_log2=5, sigma_l=1.0, sigma_z=0.01, sigma_a=0.1):
    """(linear, var) of dsrt_denoise_accumulated_coverage: alpha None is _denoise_model.denoise."""
    c, v = start(S, S2, n)
    if alpha is None:
        Fm, a = filterable(guides["range"], n), None
    else:
        a = np.asarray(alpha, F)
        Fm = coverage_filterable(guides["range"], n, a, alpha_min)
        with np.errstate(all="ignore"):
            aa = a * a
            c = np.where(Fm[..., None], c / a[..., None], c).astype(F)
            v = np.where(Fm[..., None], v / aa[..., None], v).astype(F)
    for i in range(iterations):
        c, v = iterate(c, v, Fm, guides, 1 << i, normal_power_log2, sigma_l, sigma_z, sigma_a)
    if a is not None:
        with np.errstate(all="ignore"):
            aa = a * a
            c = np.where(Fm[..., None], c * a[..., None], c).astype(F)
            v = np.where(Fm[..., None], v * aa[..., None], v).astype(F)
    return c, v
