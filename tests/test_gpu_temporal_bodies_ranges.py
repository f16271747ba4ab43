"""The motion stage's body search on the GPU (csrc/temporal_kernel.hip, dsrt_temporal_bodies_kernel) where tests/test_gpu_temporal_bodies.py does not reach: all 15
ranges of the search, all 96 float4 of the pose table in LDS and moved bits up to 15 -- sixteen body ranges, empty ones among them, every edge planted, once with
the last body empty and once with it owning pixels -- and ranges that end at 2^31 or reach beyond it.  Both forms against the numpy model of
tests/_motion_model.py, bit for bit, on all seven outputs and on `next`.  The cases are those of tests/test_temporal_bodies_ranges_host.py."""
import numpy as np
import pytest

import _bodies_model as B
import _motion_model as model
from _denoise_model import DEFAULTS as DN
from test_gpu_temporal_bodies import DEV, GUIDES, WANT_ALL, _bits, _check_frame, _desc, _dev, _dev64, _synthetic
from test_temporal_bodies_ranges_host import UNMOVED16, poses16, prims16, prims_around_2_31, ranges16, ranges_to_2_31

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

W, H = 33, 17


def _both_forms(dsrt, gpu_ctx, oracle, s, mo, what, it=1):
    """One frame with the previous frame of `s`, host form and device form, against the model: all seven outputs and next."""
    desc = _desc(dsrt, W, H)
    want = model.denoise_temporal_bodies(s["S"], s["S2"], 8, s["g"], mo, s["cam0"], s["prev"], **{**DN, "iterations": it})
    host = gpu_ctx.denoise_temporal_bodies_to_host(desc, s["S"], s["S2"], s["g"], mo, s["cam0"], s["prev"], params=dsrt.denoise_defaults(iterations=it), want_f32=True,
                                                   want_var=True, samples_done=8)
    _check_frame(oracle, host[:7], host[7], want, (what, "host form"))
    nxt = torch.full((W * H * 16,), -7.5, dtype=torch.float32, device=DEV)
    got = gpu_ctx.denoise_temporal_bodies(desc, _dev64(s["S"]), _dev64(s["S2"]), {k: _dev(s["g"][k]) for k in GUIDES}, (*mo[:4], _dev(mo[4], np.int32)), nxt, s["cam0"],
                                          _dev(s["prev"]).reshape(-1), params=dsrt.denoise_defaults(iterations=it), samples_done=8, **WANT_ALL)
    torch.cuda.synchronize()
    _check_frame(oracle, got, nxt, want, (what, "device form"))
    return want


@pytest.mark.parametrize("last_live", [False, True])
def test_sixteen_ranges_equal_the_model(dsrt, gpu_ctx, oracle, last_live):
    """The synthetic frame over 16 bodies that tile [0, 600), three of them empty (last_live: two, and the last body owns pixels); then `bodies` = 5 on the same arrays."""
    rng = np.random.default_rng(1600 + last_live)
    s = _synthetic(dsrt, rng, W, H)
    first, num = ranges16(last_live)
    s["prim"] = prims16(rng, (H, W), first, num)
    z = (0.0, 0.0, 1.0)
    pp, pc = poses16(rng, lambda: B._pose(B._rot(z, rng.uniform(-0.08, 0.08)), (rng.uniform(-0.4, 0.4), rng.uniform(-0.4, 0.4), 0.0)))    # in the wall's plane: the history blends
    body = model.body_of(s["prim"], first, num)
    assert all(((body == b).sum() > 0) == (num[b] > 0) for b in range(16))                    # every non-empty body owns pixels
    moved = model.moved_bodies(pp, pc)
    assert [b for b in range(1, 16) if not moved[b]] == list(UNMOVED16)
    want = _both_forms(dsrt, gpu_ctx, oracle, s, (first, num, pp, pc, s["prim"]), ("16 ranges", last_live))
    hit = s["g"]["range"] <= 3e38
    for b in range(1, 16):                                                                    # a moved body's pixels moved, the others kept their bits
        on = (body == b) & hit
        if on.any():
            assert (_bits(want["prev_position"])[on] != _bits(s["g"]["position"])[on]).any(axis=1).all() == bool(moved[b]), b
    assert (want["found"] & moved[body]).sum() > W * H // 8
    # the same arrays, `bodies` = 5: bodies 5 .. 15 are body 0
    want5 = _both_forms(dsrt, gpu_ctx, oracle, s, (first[:5], num[:5], pp[:5], pc[:5], s["prim"]), ("5 of 16 ranges", last_live))
    on = (body >= 5) & hit
    assert on.any() and np.array_equal(_bits(want5["prev_position"])[on], _bits(s["g"]["position"])[on])


@pytest.mark.parametrize("past", [False, True])
def test_ranges_next_to_2_31_equal_the_model(dsrt, gpu_ctx, oracle, past):
    """first_tri + num_tris == 2^31, and 90 beyond it: the kernel's range test is the header's rule for every int32 prim_id, the negative ones next to -2^31
    included (a 32-bit unsigned test alone puts -2^31 .. -2^31 + 89 on body 1 in the second case)."""
    rng = np.random.default_rng(231)
    s = _synthetic(dsrt, rng, W, H)
    first, num = ranges_to_2_31(past)
    s["prim"] = prims_around_2_31(W * H).reshape(H, W)
    pp, pc = s["poses"]["in the plane"]
    body = model.body_of(s["prim"], first, num)
    hit = s["g"]["range"] <= 3e38
    assert ((body == 1) & hit).sum() >= 5 and not body[s["prim"] < 0].any() and model.moved_bodies(pp, pc)[1] and ((s["prim"] < -2 ** 31 + 90) & hit).sum() >= 50
    want = _both_forms(dsrt, gpu_ctx, oracle, s, (first, num, pp, pc, s["prim"]), ("ranges next to 2^31", past))
    still = (body != 1) & hit
    assert np.array_equal(_bits(want["prev_position"])[still], _bits(s["g"]["position"])[still])
    assert (_bits(want["prev_position"])[(body == 1) & hit] != _bits(s["g"]["position"])[(body == 1) & hit]).any(axis=1).all()
