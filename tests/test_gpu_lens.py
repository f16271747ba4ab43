"""The lens model on the GPU (include/dsrt.h, LENS MODEL) against the numpy model of tests/_lens_model.py, bit for bit: image, src_xy and status for 1, 3 and 4
channels and the three filters at the shapes of _lens_model.CASES -- the smallest at which tile seams (64 x 4 output pixels per workgroup), partial waves, the
fold-over and the border taps all occur -- then vignetting, the clamp, an id plane through nearest, every output subset, the host form, refusals over canaries,
stream order, context state, and the CLI's chain.  Every comparison is on 32-bit words."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

from conftest import ASSETS, ROOT
import _lens_model as M
import _sensor_model as SM
from _lens_model import F

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ALL = ("image", "src_xy", "status")


def _words(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32) if a.dtype.itemsize == 4 else a


def _same(got, want, what):
    g, w = _words(got), _words(want)
    assert g.size == w.size and g.dtype == w.dtype, (what, g.shape, w.shape, g.dtype, w.dtype)
    bad = g.reshape(-1) != w.reshape(-1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at flat index {int(np.argmax(bad))}"


def _lib_params(dsrt, p):
    return dsrt.lens_defaults(**{k: (float(v) if k in M.FLOAT_FIELDS else int(v)) for k, v in p.items()})


def _source(rng, p):
    """Filters 1 and 2: a random finite float frame with negative values, exact zeros and a few -0.0f; nearest: random 32-bit words (NaN patterns among them)."""
    shape = (p["src_height"], p["src_width"], p["channels"])
    if p["filter"] == M.NEAREST:
        return rng.integers(0, 2 ** 32, shape, dtype=np.uint64).astype(np.uint32).view(np.int32)
    x = (rng.random(shape, dtype=F) * F(1.25) - F(0.25)).astype(F)
    flat = x.reshape(-1)
    flat[rng.choice(flat.size, max(2, flat.size // 9), replace=False)] = F(0.0)
    flat[rng.choice(flat.size, max(2, flat.size // 50), replace=False)] = F(-0.0)
    return x


def _check(dsrt, ctx, p, W, H, src, what, on_device=True, want=ALL):
    desc = dsrt.make_desc(W, H, 1)
    got = ctx.lens_apply(desc, torch.from_numpy(src).to(DEV) if on_device else src, _lib_params(dsrt, p), want=want)
    if on_device:
        torch.cuda.synchronize()
    model = M.apply(p, src, W, H)
    for k in want:
        _same(got[k], model[k], (what, k))
    return model


# ---- 1. the kernel against the model ----
@pytest.mark.parametrize("case", list(M.CASES))
def test_every_instantiation_matches_the_model(dsrt, gpu_ctx, case):
    rng = np.random.default_rng(sum(map(ord, case)))
    W, H, kw = M.CASES[case]
    for channels, flt in itertools.product((1, 3, 4), (M.NEAREST, M.BILINEAR, M.CUBIC)):
        p = M.params(filter=flt, channels=channels, fill_bits=0x7FC00001, **kw)
        model = _check(dsrt, gpu_ctx, p, W, H, _source(rng, p), (case, channels, flt))
        st = model["status"]
        if case == "mixed" and flt == M.CUBIC:                                                   # no branch passes vacuously
            for name, share in (("not inverted", (st == 0).mean()), ("all inside", (st == 7).mean()), ("partly inside", (st == 3).mean()), ("outside", (st == 1).mean())):
                assert share >= 0.05, (name, share)
        if case in ("barrel", "pincushion", "wide", "tiny"):
            assert (st & 1).all()
        assert not model["src_xy"][st == 0].view(np.uint32).any()


def test_two_channels_too(dsrt, gpu_ctx):
    rng = np.random.default_rng(2)
    W, H, kw = M.CASES["mixed"]
    for flt in (M.NEAREST, M.BILINEAR, M.CUBIC):
        p = M.params(filter=flt, channels=2, **kw)
        _check(dsrt, gpu_ctx, p, W, H, _source(rng, p), ("two channels", flt))


def test_vignetting_with_and_without_cos4(dsrt, gpu_ctx):
    rng = np.random.default_rng(3)
    W, H, kw = M.CASES["barrel"]
    for flt, cos4, (v1, v2, v3) in itertools.product((M.BILINEAR, M.CUBIC), (0, 1), ((-0.3, 0.05, -0.01), (-3.0, 0.0, 0.0), (0.0, 0.0, 0.0))):
        p = M.params(filter=flt, channels=3, cos4=cos4, v1=v1, v2=v2, v3=v3, **kw)
        model = _check(dsrt, gpu_ctx, p, W, H, np.abs(_source(rng, p)) + F(0.5), ("vignetting", flt, cos4, v1))
        img = model["image"].reshape(H, W, 3)
        if v1 == -3.0:
            assert (img[0, 0] == 0).all() and img[H // 2, W // 2].min() > 0                      # the gain is clamped at zero in the corners, not negative
        elif cos4 or v1:
            assert img[0, 0].max() < img[H // 2, W // 2].min() * 1.2                             # darker towards the corners
    nearest = M.params(filter=M.NEAREST, channels=1, cos4=1, v1=-0.3, **kw)                      # nearest copies words: no gain
    src = _source(rng, nearest)
    plain = M.apply(M.params(filter=M.NEAREST, channels=1, **kw), src, W, H)
    _same(_check(dsrt, gpu_ctx, nearest, W, H, src, "nearest ignores vignetting")["image"], plain["image"], "nearest with and without vignetting")


def test_clamp_zero_on_a_single_bright_texel(dsrt, gpu_ctx):
    W, H, kw = M.CASES["barrel"]
    src = np.zeros((kw["src_height"], kw["src_width"], 1), F)
    src[14, 22] = F(1.0)
    off = _check(dsrt, gpu_ctx, M.params(filter=M.CUBIC, channels=1, clamp_zero=0, **kw), W, H, src, "clamp off")["image"]
    on = _check(dsrt, gpu_ctx, M.params(filter=M.CUBIC, channels=1, clamp_zero=1, **kw), W, H, src, "clamp on")["image"]
    assert (off < 0).sum() >= 4 and off.max() > 0.5                                             # Catmull-Rom's negative lobes around the texel ...
    assert (on >= 0).all() and not np.signbit(on[off < 0]).any() and np.array_equal(on[off > 0], off[off > 0])      # ... clamp to +0; the rest is untouched
    lin = _check(dsrt, gpu_ctx, M.params(filter=M.BILINEAR, channels=1, clamp_zero=0, **kw), W, H, src, "bilinear")["image"]
    assert (lin >= 0).all()


def test_an_id_plane_goes_through_nearest_untouched(dsrt, gpu_ctx):
    W, H, kw = M.CASES["mixed"]
    sw, sh = kw["src_width"], kw["src_height"]
    ids = (np.arange(sw * sh, dtype=np.uint32) * np.uint32(2654435761)).reshape(sh, sw, 1)      # every texel its own 32-bit id, high bits set
    ids[ids == 0xFFFFFFFF] = 1
    p = M.params(filter=M.NEAREST, channels=1, fill_bits=0xFFFFFFFF, **kw)
    desc = dsrt.make_desc(W, H, 1)
    host = gpu_ctx.lens_apply(desc, ids, _lib_params(dsrt, p))                                  # uint32, the host form
    dev = gpu_ctx.lens_apply(desc, torch.from_numpy(ids.view(np.int32)).to(DEV), _lib_params(dsrt, p))      # the same words as int32, the device form
    torch.cuda.synchronize()
    model = M.apply(p, ids, W, H)
    assert host["image"].dtype == np.uint32 and dev["image"].dtype == torch.int32
    for k in ALL:
        _same(host[k], model[k], ("id plane, host form", k)); _same(dev[k], model[k], ("id plane, device form", k))
    img, st = host["image"].reshape(H, W), model["status"]
    assert (img[st != 7] == 0xFFFFFFFF).all() and np.isin(img[st == 7], ids).all() and (st == 7).mean() > 0.3 and (st != 7).mean() > 0.3
    qx, qy = np.floor(model["src_xy"][..., 0] + F(0.5)).astype(int), np.floor(model["src_xy"][..., 1] + F(0.5)).astype(int)
    assert np.array_equal(img[st == 7], ids[qy[st == 7], qx[st == 7], 0])                       # each id is the one at the rounded source position
    with pytest.raises(TypeError):
        gpu_ctx.lens_apply(desc, ids, _lib_params(dsrt, M.params(filter=M.CUBIC, channels=1, **kw)))          # words are not samples


# ---- 2. without the model ----
def test_every_output_subset_gives_the_same_bytes(dsrt, gpu_ctx):
    rng = np.random.default_rng(5)
    W, H, kw = M.CASES["mixed"]
    desc = dsrt.make_desc(W, H, 1)
    for flt in (M.NEAREST, M.CUBIC):
        p = M.params(filter=flt, channels=3, v1=-0.2, **kw)
        src = torch.from_numpy(_source(rng, p)).to(DEV)
        full = gpu_ctx.lens_apply(desc, src, _lib_params(dsrt, p), want=ALL)
        for n in (1, 2):
            for subset in itertools.combinations(ALL, n):
                part = gpu_ctx.lens_apply(desc, src, _lib_params(dsrt, p), want=subset)
                assert set(part) == set(subset)
                for k in subset:
                    _same(part[k], full[k], (flt, subset, k))


def test_the_host_form(dsrt, gpu_ctx):
    rng = np.random.default_rng(6)
    for case in ("mixed", "wide"):
        W, H, kw = M.CASES[case]
        for flt in (M.NEAREST, M.BILINEAR, M.CUBIC):
            p = M.params(filter=flt, channels=3, **kw)
            _check(dsrt, gpu_ctx, p, W, H, _source(rng, p), ("host form", case, flt), on_device=False)


def test_refusals_touch_nothing(dsrt, gpu_ctx):
    W, H, kw = M.CASES["barrel"]
    px, spx = W * H, kw["src_width"] * kw["src_height"]
    lib, ctx, capi = dsrt.lib, gpu_ctx._h, dsrt.capi
    desc = dsrt.make_desc(W, H, 1)
    arena = torch.full((spx * 12 + px * 64,), 0x5A, dtype=torch.uint8, device=DEV)               # source and outputs carved out of one canary-filled allocation
    base = arena.data_ptr()
    assert base % 4 == 0
    src, image, xy, status = base, base + spx * 12, base + spx * 12 + px * 16, base + spx * 12 + px * 32
    nan = float("nan")

    def call(ctx_=ctx, desc_=desc, src_=src, out=None, **fields):
        p = _lib_params(dsrt, M.params(**kw))
        for k, v in fields.items():
            setattr(p, k, v)
        out = capi.DsrtLensOut(image, xy, status) if out is None else out
        return lib.dsrt_lens_apply(ctx_, C.byref(desc_) if desc_ is not None else None, src_, C.byref(p), C.byref(out), None)

    refused = [dict(ctx_=None), dict(desc_=None), dict(src_=None), dict(desc_=dsrt.make_desc(1, H, 1)), dict(desc_=dsrt.make_desc(65536, 32768, 1)),
               dict(src_width=1), dict(src_height=0), dict(src_width=65536, src_height=32768), dict(fx=0.0), dict(fy=nan), dict(src_fx=-1.0), dict(src_fy=float("inf")),
               dict(cx=nan), dict(src_cy=float("inf")), dict(k1=nan), dict(k3=float("inf")), dict(p2=nan), dict(v1=nan), dict(v3=float("-inf")),
               dict(filter=3), dict(filter=-1), dict(channels=0), dict(channels=5), dict(cos4=2), dict(clamp_zero=-1),
               dict(out=capi.DsrtLensOut(None, None, None)), dict(src_=src + 2), dict(out=capi.DsrtLensOut(image + 1, None, None)), dict(out=capi.DsrtLensOut(None, xy + 2, None)),
               dict(out=capi.DsrtLensOut(src + 4, None, None)), dict(out=capi.DsrtLensOut(None, None, src + spx * 12 - 1)), dict(out=capi.DsrtLensOut(image, image + 8, None)),
               dict(out=capi.DsrtLensOut(None, xy, xy + px * 8 - 1))]
    for r in refused:
        assert call(**r) == -1, r
        assert lib.dsrt_last_error()
    torch.cuda.synchronize()
    assert bool((arena == 0x5A).all()), "a refused call wrote"
    # the host form refuses the same of its host pointers
    h_src, h_img = np.zeros(spx * 3, F), np.full(px * 3, 7.0, F)
    p = _lib_params(dsrt, M.params(**kw))
    bad = _lib_params(dsrt, M.params(**dict(kw, k2=nan)))
    out = capi.DsrtLensOut(h_img.ctypes.data, None, None)
    assert lib.dsrt_lens_apply_to_host(ctx, C.byref(desc), h_src.ctypes.data, C.byref(bad), C.byref(out)) == -1
    assert lib.dsrt_lens_apply_to_host(ctx, C.byref(desc), h_src.ctypes.data, C.byref(p), C.byref(capi.DsrtLensOut(h_src.ctypes.data + 8, None, None))) == -1
    assert (h_img == 7.0).all() and not h_src.any()
    # ... and the same pointers are fine once the parameters are: the outputs end where they should
    arena[:spx * 12].zero_()
    assert call() == 0
    torch.cuda.synchronize()
    got = arena.cpu().numpy()
    o = spx * 12
    assert (got[o + px * 12:o + px * 16] == 0x5A).all() and (got[o + px * 16 + px * 8:o + px * 32] == 0x5A).all() and (got[o + px * 32 + px:] == 0x5A).all()
    model = M.apply(M.params(**kw), np.zeros((kw["src_height"], kw["src_width"], 3), F), W, H)
    _same(got[o:o + px * 12].view(np.uint32), model["image"], "image after the refusals")
    _same(got[o + px * 16:o + px * 24].view(np.uint32), model["src_xy"], "src_xy after the refusals")
    _same(got[o + px * 32:o + px * 33], model["status"], "status after the refusals")


def _camera_params(dsrt, cam, W, H, zoom=1.0, **changes):
    """The CLI's parameters for a frame of W x H through `cam`: the camera's intrinsics on both sides, the output's focal lengths times zoom."""
    k = dsrt.lens_intrinsics_from_camera(cam, W, H)
    return M.params(src_width=W, src_height=H, src_fx=k[0], src_fy=k[1], src_cx=k[2], src_cy=k[3], fx=F(np.float64(k[0]) * zoom), fy=F(np.float64(k[1]) * zoom), cx=k[2], cy=k[3],
                    **changes)


def test_stream_order_and_a_following_render(dsrt):
    """The call waits for the context's previous launch -- the lens on another stream than the denoiser that writes its source reads the finished frame -- and it
    leaves camera, sun and buffers alone: a render after it gives the bytes of the render before."""
    from _sample_sets import parity_case
    ctx = dsrt.Context(0)
    try:
        hs, scene, W, H, spp, depth = parity_case(dsrt, "textured", 1337, 8)
        ctx.upload(scene)
        desc = dsrt.make_desc(W, H, spp, depth, seed=1337, rng_mode=1, gamma=scene.params.gamma)
        before = ctx.render_to_host(desc, want_f32=True)
        acc = dsrt.Accumulator(ctx, desc, moments=True)
        acc.render(0)
        guides = acc.guides()
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
        p = _camera_params(dsrt, scene.camera, W, H, zoom=1.1, k1=-0.3, k2=0.08, p1=0.003, v1=-0.2, cos4=1)
        _, _, lin, _ = ctx.denoise_accumulated(desc, acc.sum, acc.sum_sq, guides, samples_done=spp, stream=s1)
        got = ctx.lens_apply(desc, lin, _lib_params(dsrt, p), stream=s2)
        torch.cuda.synchronize()
        model = M.apply(p, lin.cpu().numpy(), W, H)
        assert lin.any() and model["image"].any() and (model["status"] == 7).mean() > 0.5
        for k in ALL:
            _same(got[k], model[k], ("behind the denoiser on another stream", k))
        after = ctx.render_to_host(desc, want_f32=True)
        assert before[0].any()
        _same(after[0], before[0], "rgb8 of a render after the lens call"); _same(after[1], before[1], "f32 of a render after the lens call")
    finally:
        ctx.close()


# ---- 3. the CLI's chain ----
POSES = "-298.0 706.0 -482.0   -300.0 700.0 -500.0   0.0 0.0 0.0\n"
SPEC = "k1=-0.3,k2=0.08,p1=0.003,p2=-0.002,zoom=1.1,vig=-0.2:0.02:0,cos4"
SPEC_PARAMS = dict(k1=-0.3, k2=0.08, p1=0.003, p2=-0.002, v1=-0.2, v2=0.02, cos4=1)


def _cli(tmp, poses, *flags):
    exe = os.path.join(ROOT, "deep-space-ray-tracer_amd", "dsrt_render")
    cmd = [exe, "--obj", os.path.join(ASSETS, "textured.obj"), "--input_txt", str(poses), "--width", "48", "--height", "32", "--spp", "8", "--depth", "8", "--rng-mode", "1",
           "--output_dir", str(tmp)] + list(flags)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r


def _read_pfm(path):
    data = open(path, "rb").read()
    head, dims, scale, rest = data.split(b"\n", 3)
    assert head == b"PF" and float(scale) < 0
    w, h = map(int, dims.split())
    return np.frombuffer(rest, "<f4").reshape(h, w, 3)[::-1].reshape(h, w, 3)


def _star_lines(path):
    rows = [line.split() for line in open(path).read().splitlines()]
    return (np.array([int(r[0]) for r in rows]), np.array([[F(r[1]), F(r[2])] for r in rows], F).reshape(-1, 2), np.array([int(r[3]) for r in rows], np.uint8))


def test_cli_lens_behind_the_stars_and_before_the_sensor(dsrt, gpu_ctx, tmp_path):
    W, H, spp = 48, 32, 8
    poses = tmp_path / "poses.txt"
    poses.write_text(POSES)
    ra, dec, mag = dsrt.synthetic_star_catalog(5, 20000, 0.0, 6.0)
    cat = tmp_path / "catalogue.txt"
    cat.write_text("".join(f"{a!r} {d!r} {m!r}\n" for a, d, m in zip(ra.tolist(), dec.tolist(), mag.tolist())))
    _cli(tmp_path / "plain", poses, "--lens", SPEC + ",filter=linear")
    _cli(tmp_path / "chain", poses, "--stars", f"{cat},flux=40", "--lens", SPEC, "--sensor", "psf=gauss:1.0:7,read=4,seed=3")
    base = "frame_0000"
    assert sorted(os.listdir(tmp_path / "plain")) == [base + t for t in (".ppm", "_lens.pfm", "_lens_map.pfm")]
    assert sorted(os.listdir(tmp_path / "chain")) == sorted(base + t for t in (".ppm", "_lens.pfm", "_lens_map.pfm", "_raw.ppm", "_sensor.png", "_stars.pfm", "_stars.txt", "_stars_lens.txt"))
    hs = dsrt.HostScene().add_obj(os.path.join(ASSETS, "textured.obj"))
    hs.build_bvh()
    fr = dsrt.pose_to_frame(dsrt.read_pose_file(str(poses))[0])
    cam = dsrt.frame_camera(fr, 40.0, W, H, spp, 8)
    gpu_ctx.upload(hs.view(cam, tuple(fr.sun_dir_model)))
    desc = dsrt.make_desc(W, H, spp, 8, gamma=2.0, seed=1337, rng_mode=1)
    rgb, _, lin, _, _ = gpu_ctx.render_denoised_to_host(desc, params=dsrt.denoise_defaults(iterations=0))
    assert lin.any()
    for run in ("plain", "chain"):                                                              # the frame itself is what it is without the flag
        assert open(tmp_path / run / (base + ".ppm"), "rb").read().endswith(rgb.tobytes())

    def check(run, source, p):
        got = _read_pfm(tmp_path / run / (base + "_lens.pfm"))
        lens_map = _read_pfm(tmp_path / run / (base + "_lens_map.pfm"))
        lib_out = gpu_ctx.lens_apply(desc, source, _lib_params(dsrt, p))
        model = M.apply(p, source, W, H)
        _same(got, lib_out["image"], (run, "the CLI's warped frame against the library")); _same(got, model["image"], (run, "... against the model"))
        _same(lens_map[..., :2], model["src_xy"], (run, "the map")); _same(lens_map[..., 2], model["status"].astype(F), (run, "the status plane"))
        assert (model["status"] == 7).mean() > 0.5 and got.any()
        return got

    check("plain", lin, _camera_params(dsrt, cam, W, H, zoom=1.1, filter=M.BILINEAR, **SPEC_PARAMS))
    with_stars = (lin + _read_pfm(tmp_path / "chain" / (base + "_stars.pfm"))).astype(F)        # POINT SOURCES: out = linear_in + layer, one fp32 addition
    p = _camera_params(dsrt, cam, W, H, zoom=1.1, **SPEC_PARAMS)
    warped = check("chain", with_stars, p)
    assert not np.array_equal(with_stars, lin)
    # the star labels: dsrt_lens_distort_points of the centroids the star pass wrote, for the stars it projected
    idx, xy, status = _star_lines(tmp_path / "chain" / (base + "_stars.txt"))
    idx2, xy2, status2 = _star_lines(tmp_path / "chain" / (base + "_stars_lens.txt"))
    want_xy, ok = dsrt.lens_distort_points(_lib_params(dsrt, p), xy)
    proj = (status & 1) != 0
    assert proj.sum() > 20 and ok.all() and np.array_equal(idx, idx2) and np.array_equal(status, status2)
    _same(xy2[proj], want_xy[proj], "the distorted centroids"); assert not xy2[~proj].any()
    _same(want_xy, M.distort_points(p, xy)[0], "the library's distorted centroids against the model")
    # the detector's raw frame is the warped frame's
    raw, maxval = SM.read_pnm(tmp_path / "chain" / (base + "_raw.ppm"))
    psf = dsrt.sensor_psf_gaussian(1.0, 7)
    assert maxval == 4095
    _same(raw, SM.apply(warped, psf, read_e=4.0, seed=3, frame=0)[0], "the raw frame against _sensor_model on the warped frame")
    assert not np.array_equal(raw, SM.apply(with_stars, psf, read_e=4.0, seed=3, frame=0)[0])


def test_cli_lens_in_rng_mode_0_is_announced_and_ignored(tmp_path):
    poses = tmp_path / "poses.txt"
    poses.write_text(POSES)
    exe = os.path.join(ROOT, "deep-space-ray-tracer_amd", "dsrt_render")
    r = subprocess.run([exe, "--obj", os.path.join(ASSETS, "textured.obj"), "--input_txt", str(poses), "--width", "48", "--height", "32", "--spp", "2", "--depth", "4", "--frames", "1",
                        "--output_dir", str(tmp_path / "out"), "--lens", "k1=-0.2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "--lens needs --rng-mode 1" in r.stderr and os.listdir(tmp_path / "out") == ["frame_0000.ppm"]
