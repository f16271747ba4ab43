"""The detector model on the GPU (include/dsrt.h, SENSOR MODEL) against the numpy model of tests/_sensor_model.py, bit for bit: random frames at the smallest shapes
at which tiling, halo, clipping, counter layout and clamps can each go wrong on their own, a point source without the model, every output subset, the host form,
the refusals, context state, and the CLI's one-call chain.  Every float comparison is on uint32 views."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

from conftest import ASSETS, ROOT
import _sensor_model as M
from _sensor_model import F

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED = 0xDEADBEEF00001337                       # the high word is not zero
NOISY = dict(prnu=0.02, dark_e=30.0, dsnu_e=4.0, read_e=12.0, noise=1, frame=3, seed=SEED)


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape and g.dtype == w.dtype, (what, g.shape, w.shape, g.dtype, w.dtype)
    bad = g != w
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at {np.argwhere(bad)[0].tolist()}"


def _frame(rng, W, H):
    """A random finite frame in [0, 1] with exact zeros and a few -0.0f."""
    x = rng.random((H, W, 3), dtype=F)
    flat = x.reshape(-1)
    flat[rng.choice(flat.size, max(2, flat.size // 7), replace=False)] = F(0.0)
    flat[rng.choice(flat.size, max(2, flat.size // 50), replace=False)] = F(-0.0)
    flat[0] = F(-0.0)
    return x


def _psf(rng, n):
    """Random, asymmetric, non-negative, summing to about one: a flip or a transpose changes every result."""
    taps = rng.random((n, n)).astype(F)
    taps[0, n - 1] = F(3.0)
    return (taps / taps.sum(dtype=np.float64)).astype(F)


def _run(dsrt, ctx, x, psf, on_device=True, wants=(True, True, True), **p):
    H, W, _ = x.shape
    desc = dsrt.make_desc(W, H, 1)
    params = dsrt.sensor_defaults(psf=psf, **p)
    lin = torch.from_numpy(x).to(DEV) if on_device else x
    out = ctx.sensor_apply(desc, lin, params, *wants)
    if on_device:
        torch.cuda.synchronize()
    return out


def _check(dsrt, ctx, x, psf, what, **p):
    got = _run(dsrt, ctx, x, psf, **p)
    want = M.apply(x, psf, **p)
    for g, w, name in zip(got, want, ("dn", "signal", "rgb8")):
        _same(g, w, (what, name))
    return want


# ---- 1. model parity ----
CASES = [(37, 21, n, mono) for n in (1, 3, 9, 33) for mono in (0, 1)] + [(5, 3, 33, 0), (5, 3, 33, 1), (130, 9, 33, 0), (130, 9, 33, 1), (2, 2, None, 0), (2, 2, None, 1),
                                                                         (67, 35, 5, 0)]


@pytest.mark.parametrize("W, H, n, mono", CASES)
def test_random_frames_equal_the_model(dsrt, gpu_ctx, W, H, n, mono):
    rng = np.random.default_rng(1000 * W + 10 * H + (n or 0))
    x = _frame(rng, W, H)
    psf = _psf(rng, n) if n else None
    dn, _, _ = _check(dsrt, gpu_ctx, x, psf, (W, H, n, mono, "every noise term"), mono=mono, **NOISY)
    still, _, _ = _check(dsrt, gpu_ctx, x, psf, (W, H, n, mono, "noise 0"), mono=mono, **{**NOISY, "noise": 0})
    assert not np.array_equal(dn, still)
    _check(dsrt, gpu_ctx, x, psf, (W, H, n, mono, "defaults"), mono=mono)


@pytest.mark.parametrize("mono", [0, 1])
def test_bits_saturation_and_the_zero_clamp(dsrt, gpu_ctx, mono):
    W, H = 37, 21
    rng = np.random.default_rng(5 + mono)
    x = _frame(rng, W, H)
    psf = _psf(rng, 9)
    for bits in (8, 16):
        dn, _, rgb = _check(dsrt, gpu_ctx, x, psf, ("bits", bits), mono=mono, bits=bits, e_per_dn=20000.0 / (1 << bits), **NOISY)
        assert dn.max() > (1 << bits) // 4 and rgb.max() >= 64
    blurred = M.apply(x, psf, mono=mono)[1]
    well = float(np.median(blurred)) * 20000.0                                         # about half the pixels saturate
    dn, _, _ = _check(dsrt, gpu_ctx, x, psf, "full well", mono=mono, full_well_e=well, **{**NOISY, "read_e": 2.0, "dark_e": 0.0, "dsnu_e": 0.0})
    top = dn.max()
    assert 0.3 < (dn == top).mean() < 0.7 and top < 4095
    dn, _, _ = _check(dsrt, gpu_ctx, x, psf, "negative offset", mono=mono, offset_dn=-1500.0, **NOISY)
    assert 0.1 < (dn == 0).mean() < 0.9                                                 # the zero clamp is reached, and left
    dn, _, _ = _check(dsrt, gpu_ctx, x, psf, "ADC ceiling", mono=mono, e_per_dn=1.0, **NOISY)
    assert (dn == 4095).mean() > 0.3


# ---- 2. a point source, without the model ----
def test_point_source_is_the_psf_itself(dsrt, gpu_ctx):
    n, r = 5, 2
    taps = (np.arange(n * n, dtype=F).reshape(n, n) + F(1.0)) / F(n * n * n)
    taps[0, n - 1] = F(0.3)
    value = F(0.8125)
    W, H = 70, 19                                                                       # two tiles across, two down
    for ys, xs in ((9, 40), (0, 0), (H - 1, W - 2), (1, W - 1), (15, 63), (16, 64)):     # inside; clipped by the image; across the tiles' seams
        x = np.zeros((H, W, 3), F)
        x[ys, xs] = value
        signal = _run(dsrt, gpu_ctx, x, taps, wants=(False, True, False))[1].cpu().numpy()
        want = np.zeros((H, W), F)
        for dy, dx in itertools.product(range(-r, r + 1), repeat=2):
            if 0 <= ys + dy < H and 0 <= xs + dx < W:
                want[ys + dy, xs + dx] = taps[r + dy, r + dx] * value
        for k in range(3):
            _same(np.ascontiguousarray(signal[..., k]), want, ("point source", ys, xs, k))


# ---- 3. API behaviour ----
def test_every_output_subset_and_the_host_form(dsrt, gpu_ctx):
    rng = np.random.default_rng(31)
    x, psf = _frame(rng, 37, 21), _psf(rng, 9)
    for mono in (0, 1):
        full = [t.cpu().numpy() for t in _run(dsrt, gpu_ctx, x, psf, mono=mono, **NOISY)]
        for wants in itertools.product((False, True), repeat=3):
            if not any(wants):
                continue
            for on_device in (True, False):
                got = _run(dsrt, gpu_ctx, x, psf, on_device=on_device, wants=wants, mono=mono, **NOISY)
                for g, w, want, name in zip(got, full, wants, ("dn", "signal", "rgb8")):
                    assert (g is not None) == want
                    if want:
                        _same(g, w, (mono, wants, "device" if on_device else "host", name))


def test_no_psf_is_the_unit_tap(dsrt, gpu_ctx):
    rng = np.random.default_rng(32)
    x = _frame(rng, 37, 21)
    for mono in (0, 1):
        a = _run(dsrt, gpu_ctx, x, None, mono=mono, **NOISY)
        b = _run(dsrt, gpu_ctx, x, np.ones((1, 1), F), mono=mono, **NOISY)
        for u, v, name in zip(a, b, ("dn", "signal", "rgb8")):
            _same(u, v, (mono, name))
        assert not (_bits(a[1]) == 0x80000000).any()                                    # +0 + 1 * (-0) = +0


def test_new_taps_replace_the_old_ones(dsrt, gpu_ctx):
    """The context keeps the taps on the device between calls: other taps, of the same size and of another, must reach the kernel."""
    rng = np.random.default_rng(33)
    x = _frame(rng, 37, 21)
    for n in (9, 9, 3, 33, 9):
        _check(dsrt, gpu_ctx, x, _psf(rng, n), ("taps", n), **NOISY)


def test_refusals_touch_nothing(dsrt, gpu_ctx):
    W, H = 16, 8
    px = W * H
    lib, ctx = dsrt.lib, gpu_ctx._h
    desc = dsrt.make_desc(W, H, 1)
    arena = torch.full((px * 64,), 0x5A, dtype=torch.uint8, device=DEV)                 # input and outputs carved out of one canary-filled allocation
    base = arena.data_ptr()
    assert base % 4 == 0
    lin, dn, sig, rgb = base, base + px * 16, base + px * 32, base + px * 48
    taps = np.full((3, 3), 1 / 9, F)
    good = dict(psf=taps)

    def call(ctx_=ctx, desc_=desc, lin_=lin, params=None, dn_=dn, sig_=sig, rgb_=rgb, host=False, **changes):
        p = dsrt.sensor_defaults(**{**good, **changes}) if params is None else params
        dp, pp = (C.byref(desc_) if desc_ is not None else None), (C.byref(p) if p is not False else None)
        if host:
            return lib.dsrt_sensor_apply_to_host(ctx_, dp, lin_, pp, dn_, sig_, rgb_)
        return lib.dsrt_sensor_apply(ctx_, dp, lin_, pp, dn_, sig_, rgb_, None)

    def taps_with(v):
        t = taps.copy()
        t[1, 2] = v
        return t
    nan, inf = float("nan"), float("inf")
    refused = [dict(ctx_=None), dict(desc_=None), dict(lin_=None), dict(params=False),
               dict(desc_=dsrt.make_desc(1, H, 1)), dict(desc_=dsrt.make_desc(W, 1, 1)), dict(desc_=dsrt.make_desc(65536, 32768, 1)),
               dict(psf=np.ones((2, 2), F)), dict(psf=np.ones((35, 35), F)), dict(psf=taps_with(-1e-9)), dict(psf=taps_with(nan)), dict(psf=taps_with(inf)),
               dict(gain_e=0.0), dict(gain_e=nan), dict(e_per_dn=0.0), dict(e_per_dn=-1.0), dict(e_per_dn=nan), dict(full_well_e=0.0), dict(full_well_e=nan),
               dict(prnu=-0.1), dict(prnu=nan), dict(dark_e=-1.0), dict(dark_e=nan), dict(dsnu_e=-1.0), dict(dsnu_e=nan), dict(read_e=-1.0), dict(read_e=nan),
               dict(offset_dn=inf), dict(offset_dn=-inf), dict(offset_dn=nan), dict(bits=7), dict(bits=17),
               dict(dn_=None, sig_=None, rgb_=None),
               dict(lin_=lin + 2), dict(sig_=sig + 2), dict(dn_=dn + 1),
               dict(sig_=lin), dict(dn_=lin + 8), dict(rgb_=lin + px * 12 - 1), dict(dn_=sig + 4), dict(rgb_=dn + px * 6 - 1), dict(rgb_=sig)]
    # a psf_size of 0 with taps given: the struct by hand
    p0 = dsrt.sensor_defaults(psf=taps)
    p0.psf_size = 0
    refused.append(dict(params=p0))
    for kw in refused:
        assert call(**kw) == -1, kw
        assert dsrt.lib.dsrt_last_error()
    assert bool((arena == 0x5A).all()), "a refused call wrote"
    # the host form refuses the same of its host pointers
    h_lin, h_dn = np.zeros((H, W, 3), F), np.full((H, W, 3), 0x5A5A, np.uint16)
    assert call(lin_=h_lin.ctypes.data, dn_=h_dn.ctypes.data, sig_=None, rgb_=None, host=True, bits=17) == -1
    assert call(lin_=h_lin.ctypes.data, dn_=h_lin.ctypes.data + 4, sig_=None, rgb_=None, host=True) == -1
    assert call(lin_=h_lin.ctypes.data, dn_=None, sig_=None, rgb_=None, host=True) == -1
    assert (h_dn == 0x5A5A).all() and not h_lin.any()
    # ... and the same pointers are fine once the parameters are
    arena[:px * 12].zero_()
    assert call() == 0
    torch.cuda.synchronize()
    assert int(arena[px * 12:px * 16].min()) == 0x5A == int(arena[px * 16 + px * 6:px * 32].max())      # nothing beyond the outputs' ends
    want = M.apply(np.zeros((H, W, 3), F), taps)
    _same(arena[px * 16:px * 16 + px * 6].cpu().numpy().view(np.uint16).reshape(H, W, 3), want[0], "dn after the refusals")


def test_context_state_and_a_following_render(dsrt):
    from _sample_sets import parity_case
    ctx = dsrt.Context(0)
    try:
        hs, scene, W, H, spp, depth = parity_case(dsrt, "textured", SEED, 8)
        ctx.upload(scene)
        rdesc = dsrt.make_desc(W, H, spp, depth, seed=SEED, rng_mode=1)
        before = ctx.render_to_host(rdesc, want_f32=True)
        rng = np.random.default_rng(40)
        x = _frame(rng, 50, 30)
        for n in (None, 9):
            _check(dsrt, ctx, x, _psf(rng, n) if n else None, ("with a scene resident", n), **NOISY)
        after = ctx.render_to_host(rdesc, want_f32=True)
        assert before[0].any()
        _same(after[0], before[0], "rgb8 of a render after the sensor calls"); _same(after[1], before[1], "f32 of a render after the sensor calls")
    finally:
        ctx.close()


def test_stream_order_behind_the_denoiser(dsrt):
    """The call waits for the context's previous launch: the sensor on another stream than the denoiser that writes its input reads the finished frame."""
    from _sample_sets import parity_case
    ctx = dsrt.Context(0)
    try:
        hs, scene, W, H, spp, depth = parity_case(dsrt, "textured", SEED, 8)
        ctx.upload(scene)
        desc = dsrt.make_desc(W, H, spp, depth, seed=SEED, rng_mode=1, gamma=scene.params.gamma)
        acc = dsrt.Accumulator(ctx, desc, moments=True)
        acc.render(0)
        guides = acc.guides()
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
        params = dsrt.sensor_defaults(psf=_psf(np.random.default_rng(41), 9), **NOISY)
        _, _, lin, _ = ctx.denoise_accumulated(desc, acc.sum, acc.sum_sq, guides, samples_done=spp, stream=s1)
        dn, _, _ = ctx.sensor_apply(desc, lin, params, stream=s2)
        torch.cuda.synchronize()
        _same(dn, M.apply(lin.cpu().numpy(), params._keep_psf, **NOISY)[0], "dn behind the denoiser on another stream")
    finally:
        ctx.close()


# ---- 4. the CLI's one-call chain ----
POSES = ("-298.0 706.0 -482.0   -300.0 700.0 -500.0   0.0 0.0 0.0\n" * 2)                              # two frames, one pose: the linear frames are equal, the detector's frame index is not


def _cli(tmp, poses, spec, *flags):
    exe = os.path.join(ROOT, "deep-space-ray-tracer_amd", "dsrt_render")
    cmd = [exe, "--obj", os.path.join(ASSETS, "textured.obj"), "--input_txt", str(poses), "--width", "48", "--height", "32", "--spp", "8", "--depth", "8", "--rng-mode", "1",
           "--output_dir", str(tmp), "--sensor", spec] + list(flags)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r


def test_cli_raw_frames_are_the_librarys(dsrt, gpu_ctx, tmp_path):
    W, H, spp = 48, 32, 8
    poses = tmp_path / "poses.txt"
    poses.write_text(POSES)
    spec = "psf=gauss:1.2:9,gain=18000,read=12,dark=20,prnu=0.05,dsnu=5,well=19000,epdn=5,offset=64,bits=12,seed=7"
    _cli(tmp_path / "colour", poses, spec)
    _cli(tmp_path / "still", poses, spec + ",noise=0,mono")
    assert sorted(os.listdir(tmp_path / "colour")) == sorted(f"frame_000{i}{tail}" for i in (0, 1) for tail in (".ppm", "_raw.ppm", "_sensor.png"))
    assert sorted(os.listdir(tmp_path / "still")) == sorted(f"frame_000{i}{tail}" for i in (0, 1) for tail in (".ppm", "_raw.pgm", "_sensor.png"))
    hs = dsrt.HostScene().add_obj(os.path.join(ASSETS, "textured.obj"))
    hs.build_bvh()
    fr = dsrt.pose_to_frame(dsrt.read_pose_file(str(poses))[0])
    gpu_ctx.upload(hs.view(dsrt.frame_camera(fr, 40.0, W, H, spp, 8), tuple(fr.sun_dir_model)))
    desc = dsrt.make_desc(W, H, spp, 8, gamma=2.0, seed=1337, rng_mode=1)
    rgb, _, lin, _, _ = gpu_ctx.render_denoised_to_host(desc, params=dsrt.denoise_defaults(iterations=0))
    assert lin.any()
    psf = dsrt.sensor_psf_gaussian(1.2, 9)
    p = dict(gain_e=18000.0, read_e=12.0, dark_e=20.0, prnu=0.05, dsnu_e=5.0, full_well_e=19000.0, seed=7)
    raw = []
    for i in (0, 1):
        got, maxval = M.read_pnm(tmp_path / "colour" / f"frame_000{i}_raw.ppm")
        assert maxval == 4095
        want = gpu_ctx.sensor_apply(desc, lin, dsrt.sensor_defaults(psf=psf, frame=i, **p))[0]
        _same(got, want, ("the CLI's raw frame against dsrt_sensor_apply_to_host", i))
        _same(got, M.apply(lin, psf, frame=i, **p)[0], ("the CLI's raw frame against the model", i))
        raw.append(got)
    assert not np.array_equal(raw[0], raw[1])                                           # the temporal noise changes from frame to frame ...
    still = [M.read_pnm(tmp_path / "still" / f"frame_000{i}_raw.pgm")[0] for i in (0, 1)]
    assert still[0].shape == (H, W) and np.array_equal(still[0], still[1])               # ... and the fixed pattern stays put
    _same(still[0], M.apply(lin, psf, mono=1, noise=0, frame=0, **p)[0], "the mono raw frame against the model")
    assert not np.array_equal(still[0], M.apply(lin, psf, mono=1, noise=0, frame=0, **{**p, "prnu": 0.0, "dsnu_e": 0.0})[0])


def test_cli_sensor_behind_the_denoiser_and_the_upscaler(dsrt, gpu_ctx, tmp_path):
    """The linear frame is the chosen chain's: the denoiser's (whose undenoised companion is then called _noisy) and the upscaler's, at the output size."""
    W, H, spp = 48, 32, 8
    poses = tmp_path / "poses.txt"
    poses.write_text(POSES)
    _cli(tmp_path / "dn", poses, "mono,read=5,bits=10,epdn=20", "--denoise", "1", "--frames", "1")
    _cli(tmp_path / "up", poses, "psf=gauss:0.8:3,prnu=0.01", "--upscale", "2", "--frames", "1")
    assert sorted(os.listdir(tmp_path / "dn")) == ["frame_0000.ppm", "frame_0000_noisy.ppm", "frame_0000_raw.pgm", "frame_0000_sensor.png"]
    assert sorted(os.listdir(tmp_path / "up")) == ["frame_0000.ppm", "frame_0000_lowres.ppm", "frame_0000_raw.ppm", "frame_0000_sensor.png"]
    hs = dsrt.HostScene().add_obj(os.path.join(ASSETS, "textured.obj"))
    hs.build_bvh()
    fr = dsrt.pose_to_frame(dsrt.read_pose_file(str(poses))[0])
    gpu_ctx.upload(hs.view(dsrt.frame_camera(fr, 40.0, W, H, spp, 8), tuple(fr.sun_dir_model)))
    desc = dsrt.make_desc(W, H, spp, 8, gamma=2.0, seed=1337, rng_mode=1)
    lin = gpu_ctx.render_denoised_to_host(desc, params=dsrt.denoise_defaults(iterations=1))[2]
    got, maxval = M.read_pnm(tmp_path / "dn" / "frame_0000_raw.pgm")
    assert maxval == 1023 and got.any()
    _same(got, M.apply(lin, None, mono=1, read_e=5.0, bits=10, e_per_dn=20.0)[0], "the raw frame behind the denoiser")
    big = gpu_ctx.render_upscaled_to_host(desc, 2 * W, 2 * H)[2]
    got, maxval = M.read_pnm(tmp_path / "up" / "frame_0000_raw.ppm")
    assert maxval == 4095 and got.shape == (2 * H, 2 * W, 3)
    _same(got, M.apply(big, dsrt.sensor_psf_gaussian(0.8, 3), prnu=0.01)[0], "the raw frame behind the upscaler")


def test_cli_sensor_in_rng_mode_0_is_announced_and_ignored(tmp_path):
    poses = tmp_path / "poses.txt"
    poses.write_text(POSES)
    exe = os.path.join(ROOT, "deep-space-ray-tracer_amd", "dsrt_render")
    r = subprocess.run([exe, "--obj", os.path.join(ASSETS, "textured.obj"), "--input_txt", str(poses), "--width", "48", "--height", "32", "--spp", "2", "--depth", "4", "--frames", "1",
                        "--output_dir", str(tmp_path / "out"), "--sensor", "mono"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "--sensor needs --rng-mode 1" in r.stderr and os.listdir(tmp_path / "out") == ["frame_0000.ppm"]
