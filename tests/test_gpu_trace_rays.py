"""The ray queries (include/dsrt.h, dsrt_trace_rays) on the GPU against the CPU oracle, bit for bit.

Every expected answer is dsrt_oracle_scene_hit(origin, dir, t_min, t_max) of the same ray, its derived channels (range, prim_id of a sphere,
albedo) restated in numpy float32 as tests/test_gpu_gbuffer.py does for the G-buffer.  Every float comparison is on uint32 views."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_world
from test_gpu_gbuffer import _dot, _oracle_lib, _tex2d, assert_same
from test_oracle import CASES, SUN

pytestmark = pytest.mark.gpu

F = np.float32
ALL = ("t", "range", "position", "normal", "uv", "albedo", "prim_id", "material_id", "flags")


def _sphere_roots(o, d, sph, tmin, tmax):
    """hit_sphere :478-504 in float32 for rays (o, d), one sphere and per-ray bounds: (accepted, root)."""
    c = np.array(sph["center"], F)
    r = F(sph["radius"])
    oc = o - c
    a = _dot(d, d)
    half_b = _dot(oc, d)
    cc = _dot(oc, oc) - r * r
    disc = half_b * half_b - a * cc
    ok = disc >= F(0)
    sq = np.sqrt(np.where(ok, disc, F(0)))
    with np.errstate(all="ignore"):
        root = (-half_b - sq) / a
        bad = (root < tmin) | (root > tmax)
        root2 = (-half_b + sq) / a
    root = np.where(bad, root2, root)
    ok &= ~(bad & ((root2 < tmin) | (root2 > tmax)))
    return ok, root


def expected_hits(oracle, hs, scene, O, D, TMIN=None, TMAX=None):
    """{channel: array} that the oracle's scene_hit defines for the rays (O, D) with bounds TMIN / TMAX (None: 0.001f / 1e9f)."""
    L = _oracle_lib(oracle)
    arrs = hs.arrays()
    n = len(O)
    TMIN = np.full(n, F(0.001)) if TMIN is None else TMIN
    TMAX = np.full(n, F(1e9)) if TMAX is None else TMAX
    out, ids = (C.c_float * 9)(), (C.c_int * 4)()
    T, P, N, UV = np.full(n, np.inf, F), np.zeros((n, 3), F), np.zeros((n, 3), F), np.zeros((n, 2), F)
    hit = np.zeros(n, bool)
    IDS = np.full((n, 4), -1, np.int32)
    sp = C.byref(scene)
    fp = C.POINTER(C.c_float)
    Oc, Dc = np.ascontiguousarray(O, F), np.ascontiguousarray(D, F)
    for k in range(n):
        o3 = Oc[k].ctypes.data_as(fp)
        d3 = Dc[k].ctypes.data_as(fp)
        if L.dsrt_oracle_scene_hit(sp, o3, d3, float(TMIN[k]), float(TMAX[k]), out, ids):
            hit[k] = True
            T[k], P[k], N[k], UV[k] = out[0], out[1:4], out[4:7], out[7:9]
            IDS[k] = ids[:]
    g = {"t": T, "position": P, "normal": N, "uv": UV}
    with np.errstate(all="ignore"):
        g["range"] = np.where(hit, T * np.sqrt(_dot(D, D)), F(np.inf)).astype(F)
    g["material_id"] = np.where(hit, IDS[:, 0], -1).astype(np.int32)
    prim = np.where(hit, IDS[:, 2], -1).astype(np.int32)
    sph_rays = np.nonzero(hit & (IDS[:, 2] < 0))[0]
    if sph_rays.size:                                                       # the LAST sphere whose root equals t (scene_hit keeps the last update)
        found = np.zeros(sph_rays.size, bool)
        for s, sph in enumerate(arrs["spheres"]):
            ok, root = _sphere_roots(O[sph_rays], D[sph_rays], sph, TMIN[sph_rays], TMAX[sph_rays])
            same = ok & (root.view(np.uint32) == T[sph_rays].view(np.uint32))
            prim[sph_rays[same]] = -2 - s
            found |= same
        assert found.all(), "a sphere hit the float32 restatement of hit_sphere does not reproduce"
    g["prim_id"] = prim
    alb = np.zeros((n, 3), F)
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
    g["flags"] = (hit * 1 | (hit & (IDS[:, 3] == 1)) * 2 | (hit & (IDS[:, 2] < 0)) * 4).astype(np.uint8)
    return g


def scene_box(hs):
    arrs = hs.arrays()
    pts = [arrs["tris"]["v"].reshape(-1, 3)] if len(arrs["tris"]) else []
    for s in arrs["spheres"]:
        c, r = np.array(s["center"], np.float64), abs(float(s["radius"]))
        pts.append(np.array([c - r, c + r]))
    p = np.concatenate(pts).astype(np.float64)
    return p.min(axis=0), p.max(axis=0)


def random_rays(lo, hi, n, seed):
    """Origins inside the box, on its faces and ~10^3 extents outside; directions random, toward the box, axis-aligned, with zero and -0.0 components."""
    rng = np.random.default_rng(seed)
    ext = np.maximum(hi - lo, 1e-3)
    c = 0.5 * (lo + hi)
    k = n // 3
    o_in = lo + rng.random((k, 3)) * ext
    o_face = lo + rng.random((k, 3)) * ext
    ax, side = rng.integers(0, 3, k), rng.integers(0, 2, k)
    o_face[np.arange(k), ax] = np.where(side == 1, hi[ax], lo[ax])
    u = rng.normal(size=(n - 2 * k, 3))
    o_far = c + u / np.linalg.norm(u, axis=1, keepdims=True) * (1e3 * ext.max())
    O = np.concatenate([o_in, o_face, o_far])
    target = lo + rng.random((n, 3)) * ext
    D = target - O
    D[: n // 4] = rng.normal(size=(n // 4, 3))                              # some in random directions
    D /= np.linalg.norm(D, axis=1, keepdims=True)
    pick = rng.random(n)
    axis_aligned = pick < 0.08
    e = np.eye(3)[rng.integers(0, 3, n)] * np.where(rng.random(n) < 0.5, -1.0, 1.0)[:, None]
    D[axis_aligned] = e[axis_aligned]
    zero_one = (pick >= 0.08) & (pick < 0.16)
    D[zero_one, rng.integers(0, 3, n)[zero_one]] = 0.0
    O, D = O.astype(F), D.astype(F)
    neg_zero = (D == 0) & (rng.random((n, 3)) < 0.5)
    D[neg_zero] = F(-0.0)
    perm = rng.permutation(n)
    return np.ascontiguousarray(O[perm]), np.ascontiguousarray(D[perm])


def random_ranges(first_t, seed):
    """Per-ray (t_min, t_max) around each ray's first hit at the default range: defaults, ranges that end before the first hit, a t_min past the first
    surface (the second surface is then found), and t_min > t_max."""
    rng = np.random.default_rng(seed)
    n = len(first_t)
    tmin, tmax = np.full(n, F(0.001)), np.full(n, F(1e9))
    finite = np.isfinite(first_t)
    kind = rng.integers(0, 5, n)
    cut = finite & (kind == 1)
    tmax[cut] = (first_t[cut] * F(0.5)).astype(F)
    past = finite & (kind == 2)
    tmin[past] = (first_t[past] * F(1.0001) + F(1e-3)).astype(F)
    inverted = kind == 3
    tmin[inverted], tmax[inverted] = F(10.0), F(5.0)
    exact = finite & (kind == 4) & (rng.random(n) < 0.5)
    tmax[exact] = first_t[exact]                                            # equal t is accepted
    return tmin, tmax


def _check_scene(dsrt, ctx, oracle, hs, scene, n, seed):
    ctx.upload(scene)
    lo, hi = scene_box(hs)
    O, D = random_rays(lo, hi, n, seed)
    first = ctx.trace_rays(O, D, channels=("t",))["t"]
    tmin, tmax = random_ranges(first, seed + 1)
    got = ctx.trace_rays(O, D, tmin, tmax)
    want = expected_hits(oracle, hs, scene, O, D, tmin, tmax)
    assert want["flags"].any() and not want["flags"].all()
    assert_same(got, want, keys=ALL)
    anyhit = ctx.trace_rays(O, D, tmin, tmax, any_hit=True)
    assert anyhit.keys() == {"flags"}
    assert np.array_equal(anyhit["flags"], got["flags"] & 1)                # any-hit HIT == closest-hit HIT
    return O, D, tmin, tmax, got


@pytest.mark.parametrize("name", sorted(CASES))
def test_random_rays_match_the_oracle_on_the_parity_scenes(dsrt, gpu_ctx, oracle, name):
    world, (lookfrom, lookat, vfov, W, H, depth), spp = CASES[name]
    hs = load_world(dsrt, world)
    scene = hs.view(dsrt.camera_look_at(lookfrom, lookat, vfov, W, H, spp, depth), SUN)
    _check_scene(dsrt, gpu_ctx, oracle, hs, scene, 3000, seed=sorted(CASES).index(name) * 10 + 7)


@pytest.fixture(scope="module")
def station_100k(dsrt, tmp_path_factory):
    from dsrt_amd import meshgen
    obj = tmp_path_factory.mktemp("rays") / "iss_100k.obj"
    meshgen.generate(obj, 100000)
    poses = dsrt.read_pose_file(os.path.join(GOLDEN, "rendezvous_1s_dt0_01s.txt"))
    return obj, dsrt.pose_to_frame(poses[98])


def _station(dsrt, obj, fr, kind="median", W=160, H=90):
    hs = dsrt.HostScene().add_obj(obj)
    hs.build_bvh(kind)
    return hs, hs.view(dsrt.frame_camera(fr, 40.0, W, H, 1, 50), tuple(fr.sun_dir_model))


def test_random_rays_match_the_oracle_on_the_100k_station(dsrt, gpu_ctx, oracle, station_100k):
    obj, fr = station_100k
    hs, scene = _station(dsrt, obj, fr)
    _check_scene(dsrt, gpu_ctx, oracle, hs, scene, 3000, seed=99)


@pytest.mark.parametrize("kind", ["sah", "lbvh"])
def test_other_trees_match_the_oracle_on_that_tree(dsrt, gpu_ctx, oracle, station_100k, kind):
    obj, fr = station_100k
    hs, scene = _station(dsrt, obj, fr, kind=kind)
    _check_scene(dsrt, gpu_ctx, oracle, hs, scene, 1500, seed=5 if kind == "sah" else 6)


def test_certified_tree_resident_gives_the_same_answers(dsrt, gpu_ctx, station_100k):
    obj, fr = station_100k
    hs, scene = _station(dsrt, obj, fr)
    gpu_ctx.upload(scene)
    O, D = random_rays(*scene_box(hs), 20000, seed=11)
    plain = gpu_ctx.trace_rays(O, D)
    plain_any = gpu_ctx.trace_rays(O, D, any_hit=True)
    ctx2 = dsrt.Context(0).set_certified_tree(True)
    try:
        ctx2.upload(scene)
        assert ctx2.has_certified_tree
        assert_same(ctx2.trace_rays(O, D), plain, keys=ALL)
        assert_same(ctx2.trace_rays(O, D, any_hit=True), plain_any, keys=("flags",))
    finally:
        ctx2.close()


def _pixel_centre_rays(oracle, scene, W, H):
    L = _oracle_lib(oracle)
    o3, d3 = (C.c_float * 3)(), (C.c_float * 3)()
    O, D = np.zeros((H * W, 3), F), np.zeros((H * W, 3), F)
    k = 0
    for r in range(H):
        for x in range(W):
            L.dsrt_oracle_camera_ray(C.byref(scene.camera), x, H - 1 - r, W, H, 0.5, 0.5, o3, d3)
            O[k], D[k] = o3[:], d3[:]
            k += 1
    return O, D


@pytest.mark.parametrize("where", ["station_100k", "textured", "mixed"])
def test_pixel_centre_rays_equal_the_gbuffer(dsrt, gpu_ctx, oracle, station_100k, where):
    W, H = 120, 68
    if where == "station_100k":
        obj, fr = station_100k
        hs, scene = _station(dsrt, obj, fr, W=W, H=H)
    else:
        world, (lookfrom, lookat, vfov, _, _, depth), spp = CASES[where]
        hs = load_world(dsrt, world)
        scene = hs.view(dsrt.camera_look_at(lookfrom, lookat, vfov, W, H, 1, depth), SUN)
    gpu_ctx.upload(scene)
    gb = gpu_ctx.gbuffer_to_host(dsrt.make_desc(W, H, 1))
    O, D = _pixel_centre_rays(oracle, scene, W, H)
    got = gpu_ctx.trace_rays(O, D)
    for k in ALL:
        want = gb[k].reshape((H * W,) + gb[k].shape[2:])
        if k == "flags":
            want = want & 7
        assert_same({k: got[k]}, {k: want}, keys=(k,))
    # shadow rays from those hits, as the G-buffer's shadow phase forms them: HIT == !SUN_VISIBLE wherever sun_cos > 0
    n = got["normal"]
    neg = (C.c_float * 3)(-scene.sun_dir.x, -scene.sun_dir.y, -scene.sun_dir.z)
    l3 = (C.c_float * 3)()
    _oracle_lib(oracle).dsrt_oracle_normalize(neg, l3)
    cos = gb["sun_cos"].reshape(-1)
    lit = cos > 0
    so = np.ascontiguousarray((got["position"] + n * F(1e-3))[lit], F)
    sd = np.ascontiguousarray(np.broadcast_to(np.array(l3[:], F), so.shape), F)
    blocked = gpu_ctx.trace_rays(so, sd, any_hit=True)["flags"] & 1
    visible = (gb["flags"].reshape(-1)[lit] & 8) != 0
    assert lit.sum() > 100
    assert np.array_equal(blocked == 1, ~visible)
    if where == "station_100k":
        assert blocked.any() and visible.any()


def test_batch_sizes_and_splitting(dsrt, gpu_ctx, oracle):
    import torch
    world, (lookfrom, lookat, vfov, W, H, depth), spp = CASES["station_near"]
    hs = load_world(dsrt, world)
    scene = hs.view(dsrt.camera_look_at(lookfrom, lookat, vfov, W, H, spp, depth), SUN)
    gpu_ctx.upload(scene)
    lo, hi = scene_box(hs)
    big = 3_000_000
    O, D = random_rays(lo, hi, big, seed=3)
    full = gpu_ctx.trace_rays(O, D)
    assert (full["flags"] & 1).mean() > 0.2
    # a sample of the big batch against the oracle
    idx = np.random.default_rng(4).choice(big, 800, replace=False)
    assert_same({k: v[idx] for k, v in full.items()}, expected_hits(oracle, hs, scene, O[idx], D[idx]), keys=ALL)
    # the answers do not depend on how the batch is split
    for cut in ((0, 1), (1, 64), (64, 127), (127, 192), (192, 1_000_000), (1_000_000, big)):
        a, b = cut
        part = gpu_ctx.trace_rays(np.ascontiguousarray(O[a:b]), np.ascontiguousarray(D[a:b]))
        assert_same(part, {k: v[a:b] for k, v in full.items()}, keys=ALL)
    for n in (1, 63, 65):
        part = gpu_ctx.trace_rays(np.ascontiguousarray(O[:n]), np.ascontiguousarray(D[:n]), want_stats=True)
        assert part[1].waves_launched == (n + 63) // 64 and part[1].device_flags == 0
        assert_same(part[0], {k: v[:n] for k, v in full.items()}, keys=ALL)
    # count 0 through the C ABI: DSRT_OK, nothing written
    from dsrt_amd import capi
    t = np.full(4, 7.0, F)
    rays = capi.DsrtRays(origins=O.ctypes.data, dirs=D.ctypes.data)
    hits = capi.DsrtRayHits(t=t.ctypes.data)
    st = capi.DsrtStats()
    assert dsrt.lib.dsrt_trace_rays_to_host(gpu_ctx._h, 0, C.byref(rays), 0, C.byref(hits), C.byref(st)) == 0
    assert (t == 7.0).all() and st.waves_launched == 0
    dO = torch.from_numpy(O[:64]).cuda()
    dD = torch.from_numpy(D[:64]).cuda()
    dt = torch.full((64,), 7.0, device="cuda")
    torch.cuda.synchronize()
    rays = capi.DsrtRays(origins=dO.data_ptr(), dirs=dD.data_ptr())
    hits = capi.DsrtRayHits(t=dt.data_ptr())
    assert dsrt.lib.dsrt_trace_rays(gpu_ctx._h, 0, C.byref(rays), 0, C.byref(hits), None, C.byref(st)) == 0
    assert (dt.cpu().numpy() == 7.0).all()
    assert gpu_ctx.trace_rays(O[:0], D[:0])["t"].shape == (0,)


def test_nan_and_inf_rays_leave_the_finite_rays_alone(dsrt, gpu_ctx, station_100k):
    obj, fr = station_100k
    hs, scene = _station(dsrt, obj, fr)
    gpu_ctx.upload(scene)
    O, D = random_rays(*scene_box(hs), 4000, seed=21)
    want, st0 = gpu_ctx.trace_rays(O, D, want_stats=True)
    bad_O, bad_D = O.copy(), D.copy()
    rng = np.random.default_rng(22)
    bad = rng.random(len(O)) < 0.2
    vals = np.array([np.nan, np.inf, -np.inf], F)
    for arr in (bad_O, bad_D):
        sel = bad & (rng.random(len(O)) < 0.6)
        arr[sel, rng.integers(0, 3, len(O))[sel]] = vals[rng.integers(0, 3, len(O))[sel]]
    bad_D[np.nonzero(bad)[0][:5]] = np.nan
    bad_D[np.nonzero(bad)[0][5:10]] = 0.0                                  # a zero direction as well
    bad = ~(np.isfinite(bad_O).all(axis=1) & np.isfinite(bad_D).all(axis=1) & (bad_D != 0).any(axis=1))
    assert bad.sum() > 300
    tmin = np.full(len(O), F(0.001))
    for any_hit in (False, True):
        got, st = gpu_ctx.trace_rays(bad_O, bad_D, tmin, any_hit=any_hit, want_stats=True)
        assert st.device_flags == 0
        ref = gpu_ctx.trace_rays(O, D, any_hit=True) if any_hit else want
        for k in got:
            assert_same({k: got[k][~bad]}, {k: ref[k][~bad]}, keys=(k,))


def test_errors(dsrt, gpu_ctx):
    from dsrt_amd import capi
    lib = dsrt.lib
    world, (lookfrom, lookat, vfov, W, H, depth), spp = CASES["mixed"]
    hs = load_world(dsrt, world)
    fresh = dsrt.Context(0)
    O, D = random_rays(*scene_box(hs), 64, seed=1)
    buf = np.zeros(64 * 12 + 64, np.uint8)                                    # outputs carved out of one buffer, to misalign and overlap
    t = np.zeros(64, F)
    try:
        with pytest.raises(dsrt.DsrtError) as e:
            fresh.trace_rays(O, D)
        assert e.value.code == -6                                          # DSRT_ERR_NO_SCENE
    finally:
        fresh.close()
    gpu_ctx.upload(hs.view(dsrt.camera_look_at(lookfrom, lookat, vfov, W, H, spp, depth), SUN))
    h = gpu_ctx._h

    def call(count=64, rays=None, mode=0, hits=None, null_rays=False, null_hits=False, ctx=h):
        r = None if null_rays else C.byref(rays if rays is not None else capi.DsrtRays(origins=O.ctypes.data, dirs=D.ctypes.data))
        hh = None if null_hits else C.byref(hits if hits is not None else capi.DsrtRayHits(t=t.ctypes.data))
        return lib.dsrt_trace_rays_to_host(ctx, count, r, mode, hh, None)

    assert call() == 0
    assert call(ctx=None) == -1
    assert call(null_rays=True) == -1
    assert call(null_hits=True) == -1
    assert call(rays=capi.DsrtRays(origins=None, dirs=D.ctypes.data)) == -1
    assert call(rays=capi.DsrtRays(origins=O.ctypes.data, dirs=None)) == -1
    assert call(count=-1) == -1
    assert call(mode=2) == -1 and call(mode=-1) == -1
    assert call(hits=capi.DsrtRayHits()) == -1                              # no output channel
    assert call(mode=1, hits=capi.DsrtRayHits(t=t.ctypes.data)) == -1         # any-hit: flags only
    fl = np.zeros(64, np.uint8)
    assert call(mode=1, hits=capi.DsrtRayHits(flags=fl.ctypes.data)) == 0
    base = buf.ctypes.data + (-buf.ctypes.data) % 16
    assert call(hits=capi.DsrtRayHits(t=base + 2)) == -1                      # misaligned output
    assert call(hits=capi.DsrtRayHits(flags=base + 1)) == -1
    assert call(rays=capi.DsrtRays(origins=O.ctypes.data + 2, dirs=D.ctypes.data)) == -1
    tm = np.zeros(65, F)
    assert call(rays=capi.DsrtRays(origins=O.ctypes.data, dirs=D.ctypes.data, t_min=tm.ctypes.data + 1)) == -1
    assert call(hits=capi.DsrtRayHits(t=O.ctypes.data + 4 * 100)) == -1       # output inside an input
    assert call(hits=capi.DsrtRayHits(position=D.ctypes.data - 8)) == -1
    assert call(rays=capi.DsrtRays(origins=O.ctypes.data, dirs=D.ctypes.data, t_max=tm.ctypes.data), hits=capi.DsrtRayHits(t=tm.ctypes.data + 4)) == -1
    assert lib.dsrt_trace_rays(h, 64, None, 0, None, None, None) == -1
    # the same through the Python binding
    import torch
    with pytest.raises(TypeError):
        gpu_ctx.trace_rays(O.astype(np.float64), D)
    with pytest.raises(ValueError):
        gpu_ctx.trace_rays(O[:, :2].copy(), D[:, :2].copy())
    with pytest.raises(ValueError):
        gpu_ctx.trace_rays(np.asfortranarray(O), D)
    with pytest.raises(ValueError):
        gpu_ctx.trace_rays(O, D[:10].copy())
    with pytest.raises(ValueError):
        gpu_ctx.trace_rays(O, D, channels=("depth",))
    with pytest.raises(ValueError):
        gpu_ctx.trace_rays(torch.from_numpy(O), torch.from_numpy(D))          # host tensors: not the context's device
    with pytest.raises(ValueError):
        gpu_ctx.trace_rays(torch.from_numpy(O).cuda().t().contiguous().t(), torch.from_numpy(D).cuda())
    with pytest.raises(TypeError):
        gpu_ctx.trace_rays(torch.from_numpy(O).cuda().double(), torch.from_numpy(D).cuda())
    with pytest.raises(dsrt.DsrtError):
        gpu_ctx.trace_rays(O, D, any_hit=True, channels=("t",))


def test_beauty_render_unchanged_by_a_trace_rays_call(dsrt, gpu_ctx):
    world, (lookfrom, lookat, vfov, W, H, depth), spp = CASES["station_near"]
    hs = load_world(dsrt, world)
    gpu_ctx.upload(hs.view(dsrt.camera_look_at(lookfrom, lookat, vfov, W, H, spp, depth), SUN))
    desc = dsrt.make_desc(W, H, spp, depth)
    before, f_before, _ = gpu_ctx.render_to_host(desc, want_f32=True)
    O, D = random_rays(*scene_box(hs), 5000, seed=8)
    gpu_ctx.trace_rays(O, D)
    gpu_ctx.trace_rays(O, D, any_hit=True)
    after, f_after, _ = gpu_ctx.render_to_host(desc, want_f32=True)
    assert np.array_equal(before, after) and np.array_equal(f_before.view(np.uint32), f_after.view(np.uint32))


def test_torch_on_a_stream_equals_numpy(dsrt, gpu_ctx, station_100k):
    import torch
    obj, fr = station_100k
    hs, scene = _station(dsrt, obj, fr)
    gpu_ctx.upload(scene)
    O, D = random_rays(*scene_box(hs), 50000, seed=31)
    tmin, tmax = random_ranges(gpu_ctx.trace_rays(O, D, channels=("t",))["t"], seed=32)
    want = gpu_ctx.trace_rays(O, D, tmin, tmax)
    want_any = gpu_ctx.trace_rays(O, D, tmin, tmax, any_hit=True)
    s = torch.cuda.Stream()
    dO, dD, dmin, dmax = (torch.from_numpy(x).cuda() for x in (O, D, tmin, tmax))
    got = gpu_ctx.trace_rays(dO, dD, dmin, dmax, stream=s)
    got_any = gpu_ctx.trace_rays(dO, dD, dmin, dmax, any_hit=True, stream=s)
    s.synchronize()
    assert all(isinstance(v, torch.Tensor) and v.device == dO.device for v in got.values())
    assert_same({k: v.cpu().numpy() for k, v in got.items()}, want, keys=ALL)
    assert_same({k: v.cpu().numpy() for k, v in got_any.items()}, want_any, keys=("flags",))
    # the default stream is torch's current one; a subset of channels
    sub = gpu_ctx.trace_rays(dO, dD, channels=("prim_id", "range"))
    torch.cuda.synchronize()
    assert sub.keys() == {"prim_id", "range"}
    plain = gpu_ctx.trace_rays(O, D, channels=("prim_id", "range"))
    assert_same({k: v.cpu().numpy() for k, v in sub.items()}, plain, keys=("prim_id", "range"))
