#!/usr/bin/env python3
"""What the temporal accumulation stage costs (include/dsrt.h, TEMPORAL ACCUMULATION): the station of tests/golden/assets at 1920 x 1080,
two frames of a moving camera at 8 spp, and -- HIP events around the calls, 3 warm-ups + 30 reps, medians --
    dsrt_denoise_accumulated with 0 and 1 iterations   (their difference: one a-trous iteration, step 1)
    dsrt_denoise_temporal    with 0 iterations         (its difference to the first: the temporal kernel)
One JSON line on stdout.

--bodies: the same station with a visitor -- a cube of 8 m as movable body 1, halfway between the camera and the station, about a sixth of the picture -- that turns
and shifts between the two frames (include/dsrt.h, TEMPORAL ACCUMULATION WITH BODIES), and on the second frame, in the same run,
    dsrt_denoise_temporal         with 0 iterations    (dsrt_temporal_kernel: the static stage on the same inputs)
    dsrt_denoise_temporal_bodies  with 0 iterations    (dsrt_temporal_bodies_kernel), without and with d_prev_position
each less dsrt_denoise_accumulated with 0 iterations, and the ratio of the two kernels.

--shading: the --bodies measurement as it stands, and in the same run, interleaved rep by rep (include/dsrt.h, TEMPORAL ACCUMULATION THAT FOLLOWS SHADING),
    dsrt_denoise_temporal_shaded  with 0 iterations    (dsrt_temporal_shaded_kernel) at edge_guard 0 and 1, without and with d_status
as ratios to dsrt_temporal_bodies_kernel; the shares of the pixels with geometric history that the status byte says are lost to the tap test and to the edge guards;
and what the flags channel -- it traces the shadow rays -- adds to the G-buffer call of the convenience form (normal, position, albedo, range, prim_id)."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _timed(torch, calls, warm=3, reps=30):
    """{name: [ms]} of the calls, interleaved, HIP events around each; the last call's result."""
    ms = {k: [] for k in calls}
    out = None
    for rep in range(warm + reps):
        for k, call in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = call()
            e1.record()
            e1.synchronize()
            if rep >= warm:
                ms[k].append(e0.elapsed_time(e1))
    return ms, out


def main_bodies(shading=False):
    import numpy as np
    import torch
    import dsrt_amd as d
    from conftest import load_world
    from _bodies_model import _pose, _rot
    W, H, spp, seed = 1920, 1080, 8, 0xDEADBEEF00001337
    sun = (0.32780463, -0.7564221, 0.5660121)
    eyes = ((12.4, 9.0, 37.8), (12.0, 9.0, 38.0))
    cams = [d.camera_look_at(p, (0, 0, 0), 40.0, W, H, spp, 50) for p in eyes]
    hs = load_world(d, "station_3k")
    assert hs.begin_body() == 1
    v = np.array([(x, y, z) for x in (-4, 4) for y in (-4, 4) for z in (-4, 4)], np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    t = np.zeros(12, d.capi.TRI_DTYPE)
    t["v"] = np.array([[v[a], v[b], v[c]] for q in quads for a, b, c in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))], np.float32)
    fn = np.cross(t["v"][:, 1] - t["v"][:, 0], t["v"][:, 2] - t["v"][:, 0])
    t["n"] = np.repeat((fn / np.linalg.norm(fn, axis=1, keepdims=True))[:, None, :], 3, axis=1)
    t["albedo_tex"] = -1
    mats = np.zeros(1, d.capi.MAT_DTYPE)
    mats["albedo_tex"], mats["albedo"], mats["ref_idx"] = -1, (0.7, 0.6, 0.5), 1.5
    hs.add_arrays(tris=t, mats=mats)
    hs.build_bvh_bodies()
    first, num = (np.array(x, np.int32) for x in zip(*[hs.body_range(b) for b in range(2)]))
    poses = [np.stack([np.zeros(12, np.float32), _pose(_rot((1, 2, 3), 0.5 + 0.03 * k), 0.5 * np.array(eyes[k]) + (0.3 * k, 0.2 * k, 0.0))]) for k in range(2)]
    ctx = d.Context(0)
    ctx.upload_bodies(hs, hs.view(cams[0], sun))
    hist = [torch.zeros(W * H * 16, dtype=torch.float32, device="cuda:0") for _ in range(2)]
    p0 = d.denoise_defaults(iterations=0)
    for f, cam in enumerate(cams):
        ctx.set_body_poses(1, poses[f][1:])
        ctx.set_camera_sun(cam, sun)
        desc = d.make_desc(W, H, spp, seed=seed + f, rng_mode=1)
        acc = d.Accumulator(ctx, desc, moments=True)
        acc.render(0)
        g = acc.guides()
        prim = torch.empty((H, W), dtype=torch.int32, device="cuda:0")
        flags = torch.empty((H, W), dtype=torch.uint8, device="cuda:0")
        ctx.render_gbuffer(desc, {"prim_id": prim.data_ptr(), "flags": flags.data_ptr()}, stream=ctx._raw_stream(None))
        if f == 0 and shading:                                             # (the first frame's records carry their sun state; the two older kernels do not look at it)
            ctx.denoise_temporal_shaded(desc, acc.sum, acc.sum_sq, g, flags, hist[0], (first, num, poses[0], poses[0], prim), 1, samples_done=spp, params=p0)
        elif f == 0:
            ctx.denoise_temporal_bodies(desc, acc.sum, acc.sum_sq, g, (first, num, poses[0], poses[0], prim), hist[0], samples_done=spp, params=p0)
    torch.cuda.synchronize()
    mo = (first, num, poses[0], poses[1], prim)
    calls = {
        "denoise_0_iterations": lambda: ctx.denoise_accumulated(desc, acc.sum, acc.sum_sq, g, samples_done=spp, params=p0),
        "temporal_0_iterations": lambda: ctx.denoise_temporal(desc, acc.sum, acc.sum_sq, g, hist[1], cams[0], hist[0], samples_done=spp, params=p0, want_weight=True),
        "temporal_bodies_0_iterations": lambda: ctx.denoise_temporal_bodies(desc, acc.sum, acc.sum_sq, g, mo, hist[1], cams[0], hist[0], samples_done=spp, params=p0, want_weight=True),
        "temporal_bodies_prev_position_0_iterations": lambda: ctx.denoise_temporal_bodies(desc, acc.sum, acc.sum_sq, g, mo, hist[1], cams[0], hist[0], samples_done=spp, params=p0,
                                                                                          want_weight=True, want_prev_position=True),
    }
    shaded = lambda guard, status: lambda: ctx.denoise_temporal_shaded(desc, acc.sum, acc.sum_sq, g, flags, hist[1], mo, guard, cams[0], hist[0], samples_done=spp,   # noqa: E731
                                                                       params=p0, want_weight=True, want_status=status)
    if shading:
        calls.update({f"temporal_shaded_guard{guard}{'_status' if status else ''}_0_iterations": shaded(guard, status) for guard in (0, 1) for status in (False, True)})
    ms, _ = _timed(torch, calls)
    med = {k: statistics.median(x) for k, x in ms.items()}
    w_static = calls["temporal_0_iterations"]()[5]
    w_bodies = calls["temporal_bodies_0_iterations"]()[5]
    torch.cuda.synchronize()
    on_body = prim >= int(first[1])
    k_static, k_bodies, k_pos = (med[k] - med["denoise_0_iterations"] for k in ("temporal_0_iterations", "temporal_bodies_0_iterations", "temporal_bodies_prev_position_0_iterations"))
    res = {"width": W, "height": H, "spp": spp, "body_share_of_pixels": float(on_body.float().mean()),
           "history_share_on_the_body": {"static": float((w_static[on_body] > spp).float().mean()), "bodies": float((w_bodies[on_body] > spp).float().mean())},
           "ms_median": med, "ms_min": {k: min(x) for k, x in ms.items()}, "temporal_kernel_ms": k_static, "temporal_bodies_kernel_ms": k_bodies,
           "temporal_bodies_kernel_with_prev_position_ms": k_pos, "ratio_bodies_to_static": k_bodies / k_static, "ratio_with_prev_position": k_pos / k_static}
    if shading:
        res["ratio_shaded_to_bodies"] = {k[len("temporal_shaded_"):-len("_0_iterations")]: (med[k] - med["denoise_0_iterations"]) / k_bodies for k in calls if k.startswith("temporal_shaded_")}
        st0, st1 = shaded(0, True)()[7], shaded(1, True)()[7]
        torch.cuda.synchronize()
        geo = (st1 & 4) != 0
        res["status_shares_of_pixels_with_geometric_history"] = {
            "pixels": int(geo.sum()), "share_of_image": float(geo.float().mean()), "keep_history": float(((st1 & 2) != 0)[geo].float().mean()),
            "lost_to_shading": float(((st1 & 2) == 0)[geo].float().mean()), "lost_to_the_tap_test": float(((st0 & 2) == 0)[geo].float().mean()),
            "lost_to_an_edge_guard": float((((st0 & 2) != 0) & ((st1 & 2) == 0))[geo].float().mean())}
        # the G-buffer call of the convenience form, without and with the flags channel
        chan = {k: torch.empty((H, W, 3) if k != "range" else (H, W), dtype=torch.float32, device="cuda:0") for k in ("normal", "position", "albedo", "range")}
        base = {**{k: t.data_ptr() for k, t in chan.items()}, "prim_id": prim.data_ptr()}
        gms, _ = _timed(torch, {"gbuffer_without_flags": lambda: ctx.render_gbuffer(desc, base, stream=ctx._raw_stream(None)),
                                "gbuffer_with_flags": lambda: ctx.render_gbuffer(desc, {**base, "flags": flags.data_ptr()}, stream=ctx._raw_stream(None))})
        res["gbuffer_ms_median"] = {k: statistics.median(x) for k, x in gms.items()}
        res["gbuffer_flags_adds_ms"] = res["gbuffer_ms_median"]["gbuffer_with_flags"] - res["gbuffer_ms_median"]["gbuffer_without_flags"]
    print(json.dumps(res))
    ctx.close()


def main():
    import torch
    import dsrt_amd as d
    from conftest import load_world
    W, H, spp, seed = 1920, 1080, 8, 0xDEADBEEF00001337
    hs = load_world(d, "station_3k")
    sun = (0.32780463, -0.7564221, 0.5660121)
    cams = [d.camera_look_at(p, (0, 0, 0), 40.0, W, H, spp, 50) for p in ((12.4, 9.0, 37.8), (12.0, 9.0, 38.0))]
    ctx = d.Context(0)
    ctx.upload(hs.view(cams[0], sun))
    td = d.TemporalDenoiser(ctx, d.make_desc(W, H, spp, rng_mode=1))
    p0, p1 = d.denoise_defaults(iterations=0), d.denoise_defaults(iterations=1)
    for f, cam in enumerate(cams):
        ctx.set_camera_sun(cam, sun)
        desc = d.make_desc(W, H, spp, seed=seed + f, rng_mode=1)
        acc = d.Accumulator(ctx, desc, moments=True)
        acc.render(0)
        g = acc.guides()
        if f == 0:
            td.step(acc, cam, guides=g, params=p0)
    torch.cuda.synchronize()
    prev, nxt = td.history[td.current], td.history[td.current ^ 1]
    calls = {
        "denoise_0_iterations": lambda: ctx.denoise_accumulated(desc, acc.sum, acc.sum_sq, g, samples_done=spp, params=p0),
        "denoise_1_iteration": lambda: ctx.denoise_accumulated(desc, acc.sum, acc.sum_sq, g, samples_done=spp, params=p1),
        "temporal_0_iterations": lambda: ctx.denoise_temporal(desc, acc.sum, acc.sum_sq, g, nxt, cams[0], prev, samples_done=spp, params=p0, want_weight=True),
    }
    ms = {k: [] for k in calls}
    for rep in range(33):
        for k, call in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = call()
            e1.record()
            e1.synchronize()
            if rep >= 3:
                ms[k].append(e0.elapsed_time(e1))
    med = {k: statistics.median(v) for k, v in ms.items()}
    weight = out[5]
    filt = torch.isfinite(g["range"])
    res = {"width": W, "height": H, "spp": spp, "filterable_share": float(filt.float().mean()), "history_share_of_filterable": float((weight[filt] > spp).float().mean()),
           "ms_median": med, "ms_min": {k: min(v) for k, v in ms.items()}, "atrous_iteration_ms": med["denoise_1_iteration"] - med["denoise_0_iterations"],
           "temporal_kernel_ms": med["temporal_0_iterations"] - med["denoise_0_iterations"]}
    print(json.dumps(res))
    ctx.close()


if __name__ == "__main__":
    main_bodies("--shading" in sys.argv[1:]) if {"--bodies", "--shading"} & set(sys.argv[1:]) else main()
