"""The _to_host forms of the sample-set entry points that have no Python binding -- dsrt_render_accumulate_to_host, dsrt_resolve_accumulated_to_host,
dsrt_render_accumulate_masked_to_host, dsrt_render_adaptive_to_host -- against their device forms on device buffers copied back, byte for byte.  One small
frame, 20 x 12 (neither side a multiple of the 8-pixel tile: the partial last tile column and row are in play), 6 samples per pixel, rng_mode 1."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_world
from test_oracle import SUN
from _sample_sets import SetOracle
from _adaptive_model import select_unconverged

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

SEED = 0xDEADBEEF00001337
DEV = "cuda:0"
W, H, SPP = 20, 12, 6
SET = (1, 2, 3)                                  # first, count, stride: samples 1 and 4
# Half way in from smoke()'s look-from (25, 18, 70), chosen on the CPU (test_adaptive_frame_is_the_device_forms checks the choice with the model): the station
# covers part of the frame, the last row and the last tile column included, so a tolerance of 0 keeps some pixels active and lets the others go.
LOOKFROM = (12.5, 9.0, 35.0)
PASSES, MIN_PASSES = 3, 1


def _ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def _dev64(a):
    return torch.from_numpy(np.array(a, np.uint64).reshape(-1).view(np.int64)).to(DEV)        # (a copy: the shared sums are read-only)


def _u64(t):
    return t.cpu().numpy().view(np.uint64).reshape(H, W, 3)


def _u32(t):
    return t.cpu().numpy().view(np.uint32).reshape(H, W)


@pytest.fixture(scope="module")
def frame(dsrt, gpu_ctx):
    """(scene, desc, S0, S20): the station uploaded, and sums that are not zero to add into -- sample 0 of every pixel, rendered once by the device form."""
    hs = load_world(dsrt, "station_3k")
    scene = hs.view(dsrt.camera_look_at(LOOKFROM, (0.0, 0.0, 0.0), 40.0, W, H, SPP, 50), SUN)
    scene.seed = SEED
    gpu_ctx.upload(scene)
    desc = dsrt.make_desc(W, H, SPP, 50, seed=SEED, rng_mode=1)
    acc = dsrt.Accumulator(gpu_ctx, desc, moments=True)
    acc.render(0, 1, 1)
    torch.cuda.synchronize()
    S0, S20 = _u64(acc.sum), _u64(acc.sum_sq)
    assert S0.any() and S20.any()
    S0.setflags(write=False)
    S20.setflags(write=False)
    yield scene, desc, S0, S20
    del hs


@pytest.mark.parametrize("moments", [True, False])
def test_strided_set_into_nonzero_sums_and_its_resolve(dsrt, gpu_ctx, frame, moments):
    scene, desc, S0, S20 = frame
    lib, capi = dsrt.lib, dsrt.capi
    s, sq = _dev64(S0), (_dev64(S20) if moments else None)
    gpu_ctx.render_accumulate(desc, *SET, s, sq)
    torch.cuda.synchronize()
    hs, hsq = S0.copy(), (S20.copy() if moments else None)
    acc = capi.DsrtAccum(_ptr(hs), _ptr(hsq))
    assert lib.dsrt_render_accumulate_to_host(gpu_ctx._h, C.byref(desc), *SET, C.byref(acc), None) == 0, lib.dsrt_last_error()
    assert np.array_equal(hs, _u64(s))
    assert (hs >= S0).all() and (hs > S0).any()                                     # added to what was there, not written over it
    if moments:
        assert np.array_equal(hsq, _u64(sq)) and (hsq >= S20).all() and (hsq > S20).any()
    # the resolve of those sums (samples 0, 1 and 4: three per pixel); the variance needs the second moment
    done = 1 + SET[1]
    want = gpu_ctx.resolve_accumulated(desc, s, done, sq, want_rgb8=True, want_f32=True, want_var=moments)
    torch.cuda.synchronize()
    rgb, f32 = np.zeros((H, W, 3), np.uint8), np.zeros((H, W, 3), np.float32)
    var = np.zeros((H, W, 3), np.float32) if moments else None
    assert lib.dsrt_resolve_accumulated_to_host(gpu_ctx._h, C.byref(desc), C.byref(acc), done, _ptr(rgb), _ptr(f32), _ptr(var)) == 0, lib.dsrt_last_error()
    assert rgb.any() and np.array_equal(rgb, want[0].cpu().numpy())
    assert np.array_equal(f32.view(np.uint32), want[1].cpu().numpy().view(np.uint32))
    if moments:
        assert var.any() and np.array_equal(var.view(np.uint32), want[2].cpu().numpy().view(np.uint32))
    assert np.array_equal(hs, _u64(s)) and (not moments or np.array_equal(hsq, _u64(sq)))      # the resolve reads the host sums and leaves them


def test_masked_set_with_nonzero_counts(dsrt, gpu_ctx, frame):
    scene, desc, S0, S20 = frame
    lib, capi = dsrt.lib, dsrt.capi
    yy, xx = np.mgrid[0:H, 0:W]
    mask = (((xx + yy) & 1) * 7).astype(np.uint8)                                   # a checkerboard (any nonzero byte is "set") ...
    mask[H - 1] = 0                                                                 # ... and a last row that is masked off entirely
    n0 = (np.arange(W * H, dtype=np.uint32) % 1000 + 5).reshape(H, W)
    s, sq, n = _dev64(S0), _dev64(S20), torch.from_numpy(n0.view(np.int32).copy()).to(DEV)
    gpu_ctx.render_accumulate_masked(desc, *SET, s, sq, torch.from_numpy(mask).to(DEV), n)
    torch.cuda.synchronize()
    hs, hsq, hn, hmask = S0.copy(), S20.copy(), n0.copy(), mask.copy()
    acc = capi.DsrtAccum(_ptr(hs), _ptr(hsq))
    rc = lib.dsrt_render_accumulate_masked_to_host(gpu_ctx._h, C.byref(desc), *SET, C.byref(acc), _ptr(hmask), _ptr(hn), None)
    assert rc == 0, lib.dsrt_last_error()
    assert np.array_equal(hs, _u64(s)) and np.array_equal(hsq, _u64(sq)) and np.array_equal(hn, _u32(n))
    on = mask != 0
    assert np.array_equal(hn, n0 + np.uint32(SET[1]) * on.astype(np.uint32))        # the counts move where the mask is set and nowhere else
    assert np.array_equal(hs[~on], S0[~on]) and np.array_equal(hsq[~on], S20[~on]) and (hs[on] > S0[on]).any()
    assert np.array_equal(hmask, mask)                                              # the mask is an input


def _model_active(scene, sets):
    """DsrtAdaptiveStats.active of the adaptive frame as the CPU models have it: the set oracle's sums pass by pass, the convergence test's model between them."""
    S, S2, n = np.zeros((H, W, 3), np.uint64), np.zeros((H, W, 3), np.uint64), np.zeros((H, W), np.uint32)
    active, per_pass = np.ones((H, W), bool), []
    for p in range(PASSES):
        if not active.any():
            break
        count = len(range(p, SPP, PASSES))
        a, a2 = sets.sums(scene, W, H, p, count, PASSES)
        S += a * active[..., None].astype(np.uint64)
        S2 += a2 * active[..., None].astype(np.uint64)
        n += np.uint32(count) * active.astype(np.uint32)
        per_pass.append(int(active.sum()))
        if MIN_PASSES <= p + 1 < PASSES:
            active = select_unconverged(S, S2, n, 0.0, 0.0) != 0
    return per_pass


def test_adaptive_frame_is_the_device_forms(dsrt, gpu_ctx, frame):
    """rel_tol = 0: a pixel that sees geometry never converges, a background pixel (no variance at all) converges at the first test."""
    scene, desc, _, _ = frame
    lib, capi = dsrt.lib, dsrt.capi
    model = _model_active(scene, SetOracle())
    assert len(model) == PASSES > MIN_PASSES and 0 < model[-1] < W * H, model       # the camera was chosen for this: masked passes run, over part of the frame
    ad = capi.DsrtAdaptive(PASSES, MIN_PASSES, 0.0, 0.0)
    acc = dsrt.Accumulator(gpu_ctx, desc, moments=True, counts=True)
    rgb, var = torch.zeros((H, W, 3), dtype=torch.uint8, device=DEV), torch.zeros((H, W, 3), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    dev = lambda t: C.c_void_p(t.data_ptr())                                        # noqa: E731
    st = capi.DsrtAdaptiveStats()
    rc = lib.dsrt_render_adaptive(gpu_ctx._h, C.byref(desc), C.byref(ad), C.byref(capi.DsrtAccum(dev(acc.sum), dev(acc.sum_sq))), dev(acc.n), dev(rgb), None, dev(var),
                                  None, C.byref(st))
    assert rc == 0, lib.dsrt_last_error()
    torch.cuda.synchronize()
    hst = capi.DsrtAdaptiveStats()
    hn, hrgb, hvar = np.zeros((H, W), np.uint32), np.zeros((H, W, 3), np.uint8), np.zeros((H, W, 3), np.float32)
    rc = lib.dsrt_render_adaptive_to_host(gpu_ctx._h, C.byref(desc), C.byref(ad), _ptr(hn), _ptr(hrgb), None, _ptr(hvar), C.byref(hst))
    assert rc == 0, lib.dsrt_last_error()
    # a masked pass really ran, and not over every pixel
    run = list(hst.active[:hst.passes_run])
    assert hst.passes_run > MIN_PASSES and 0 < run[-1] < W * H, (hst.passes_run, run)
    assert np.array_equal(hn, _u32(acc.n)) and len(np.unique(hn)) > 1
    assert hrgb.any() and np.array_equal(hrgb, rgb.cpu().numpy())
    assert hvar.any() and np.array_equal(hvar.view(np.uint32), var.cpu().numpy().view(np.uint32))
    # the whole DsrtAdaptiveStats, the entries past passes_run included
    assert (hst.passes_run, hst.samples_total, list(hst.active)) == (st.passes_run, st.samples_total, list(st.active))
    assert hst.samples_total == int(hn.sum()) and run == model


def test_refusals_with_a_scene_resident_leave_the_host_buffers_alone(dsrt, gpu_ctx, frame):
    """One refusal per class for each of the four forms (tests/test_host_forms_host.py has them without a device: there the accumulate forms, which ask for
    the scene first, answer DSRT_ERR_NO_SCENE): with the scene uploaded every one is DSRT_ERR_INVALID."""
    from test_host_forms_host import host_form_refusals
    host_form_refusals(dsrt, gpu_ctx._h, {"NULL": -1, "rng_mode 0": -1, "shards": -1, "width 1": -1})
