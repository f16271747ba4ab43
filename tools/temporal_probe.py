#!/usr/bin/env python3
"""What the temporal accumulation stage costs (include/dsrt.h, TEMPORAL ACCUMULATION): the station of tests/golden/assets at 1920 x 1080,
two frames of a moving camera at 8 spp, and -- HIP events around the calls, 3 warm-ups + 30 reps, medians --
    dsrt_denoise_accumulated with 0 and 1 iterations   (their difference: one a-trous iteration, step 1)
    dsrt_denoise_temporal    with 0 iterations         (its difference to the first: the temporal kernel)
One JSON line on stdout."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


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
    main()
