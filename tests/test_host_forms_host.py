"""The four _to_host forms of the sample-set entry points that have no Python binding (dsrt_render_accumulate_to_host, dsrt_resolve_accumulated_to_host,
dsrt_render_accumulate_masked_to_host, dsrt_render_adaptive_to_host) without a GPU: what they refuse, before the context or any buffer is looked at.
tests/test_gpu_host_forms.py holds them to their device forms."""
import ctypes as C

import numpy as np


def host_form_refusals(dsrt, ctx, want):
    """One refusal per class -- want = {"NULL", "rng_mode 0", "shards", "width 1": return code} -- for each of the four _to_host forms that have no Python
    binding; host buffers that hold a pattern hold it afterwards.  tests/test_gpu_host_forms.py passes a context with a scene."""
    from dsrt_amd import capi
    lib = dsrt.lib
    W, H, spp = 20, 12, 6
    good = dsrt.make_desc(W, H, spp, rng_mode=1)
    descs = {"rng_mode 0": dsrt.make_desc(W, H, spp, rng_mode=0), "shards": dsrt.make_desc(W, H, spp, rng_mode=1, shard_count=2),
             "width 1": dsrt.make_desc(1, H, spp, rng_mode=1)}
    pattern = lambda dt, n, k: (np.arange(n, dtype=np.uint64) * np.uint64(k) + np.uint64(3)).astype(dt)          # noqa: E731
    before = {"sum": pattern(np.uint64, W * H * 3, 7), "sq": pattern(np.uint64, W * H * 3, 11), "n": pattern(np.uint32, W * H, 5), "mask": pattern(np.uint8, W * H, 1),
              "rgb": pattern(np.uint8, W * H * 3, 13), "f32": pattern(np.float32, W * H * 3, 17), "var": pattern(np.float32, W * H * 3, 19)}
    b = {k: v.copy() for k, v in before.items()}
    p = {k: C.c_void_p(v.ctypes.data) for k, v in b.items()}
    acc = capi.DsrtAccum(p["sum"], p["sq"])
    ad = capi.DsrtAdaptive(3, 1, 0.0, 0.0)
    forms = {
        "accumulate": lambda c, d: lib.dsrt_render_accumulate_to_host(c, d, 1, 2, 3, C.byref(acc), None),
        "resolve": lambda c, d: lib.dsrt_resolve_accumulated_to_host(c, d, C.byref(acc), 3, p["rgb"], p["f32"], p["var"]),
        "masked": lambda c, d: lib.dsrt_render_accumulate_masked_to_host(c, d, 1, 2, 3, C.byref(acc), p["mask"], p["n"], None),
        "adaptive": lambda c, d: lib.dsrt_render_adaptive_to_host(c, d, C.byref(ad), p["n"], p["rgb"], p["f32"], p["var"], None),
    }
    got = {}
    for form, call in forms.items():
        got[form, "NULL ctx"] = (call(None, C.byref(good)), want["NULL"])
        got[form, "NULL desc"] = (call(ctx, None), want["NULL"])
        for what, desc in descs.items():
            got[form, what] = (call(ctx, C.byref(desc)), want[what][form] if isinstance(want[what], dict) else want[what])
    assert {k: v for k, v in got.items() if v[0] != v[1]} == {}
    assert lib.dsrt_last_error()
    assert all(np.array_equal(b[k].view(np.uint8), before[k].view(np.uint8)) for k in b)


def test_host_forms_refuse_without_a_device(dsrt):
    """The four _to_host forms without a Python binding, on a zeroed 64-byte stand-in for the context: a NULL argument is DSRT_ERR_INVALID everywhere; a
    bad desc is DSRT_ERR_INVALID where the form looks at desc first (the resolve, the adaptive driver), and DSRT_ERR_NO_SCENE from the two accumulate
    forms, which ask for the scene first (the stand-in has none).  Nothing is written either way."""
    ctx = C.cast(C.create_string_buffer(64), C.c_void_p)
    by_form = {"accumulate": -6, "masked": -6, "resolve": -1, "adaptive": -1}
    host_form_refusals(dsrt, ctx, {"NULL": -1, "rng_mode 0": by_form, "shards": by_form, "width 1": by_form})
