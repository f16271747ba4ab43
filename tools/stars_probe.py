#!/usr/bin/env python3
"""Measurement (not a test): what the star field costs (include/dsrt.h, POINT SOURCES) at 1920x1080 and 3840x2160 on the test suite's station mesh (pose frame 98)
for synthetic whole-sky catalogues of 2^13 and 2^20 stars.  Device times are HIP-event times on one stream around the operation, `--reps` launches after
`--warmup`, configurations interleaved rep by rep; median, min and max.  Per size and catalogue:
  stars            dsrt_render_stars with occlusion, writing linear_out, xy and status: clear, project, trace and deposit, resolve
  labels           the same writing xy and status only: project and trace -- no accumulator, nothing cleared or resolved
  no_occlusion     `stars` with occlusion = 0: no walk
  empty            `stars` with count = 0: the resolve alone (it reads the whole accumulator and puts back the zeros, so no call clears it)
  -> phase split   resolve = empty;  walk = stars - no_occlusion;  project + deposit = no_occlusion - empty
  composition      what the library offered before this pass for the same job, in the same process: dsrt_trace_rays in DSRT_TRACE_ANY mode on the in-window rays
                   (selected and packed beforehand, outside the timing: the projection and the splat are NOT in this figure) plus one full-frame device add
                   (out = linear + layer, a torch kernel).  `composition_trace` and `composition_add` are its two parts.
  spread           per configuration max - min over the repetitions: what a difference between two medians has to exceed to mean anything
Prints one JSON line.

usage: tools/stars_probe.py [--reps 15] [--warmup 3] [--frame 98]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((1920, 1080), (3840, 2160))
COUNTS = (1 << 13, 1 << 20)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frame", type=int, default=98)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import dsrt_amd as d

    say = lambda what: print(f"[stars_probe] {what}", file=sys.stderr, flush=True)   # noqa: E731
    assets = os.path.join(ROOT, "tests", "golden")
    hs = d.HostScene().add_obj(os.path.join(assets, "assets", "station_3k.obj"))
    hs.build_bvh()
    pose = d.read_pose_file(os.path.join(assets, "rendezvous_1s_dt0_01s.txt"))[a.frame]
    fr = d.pose_to_frame(pose)
    ctx = d.Context(0)
    scene = hs.view(d.frame_camera(fr, 40.0, SIZES[0][0], SIZES[0][1], 2, 50), tuple(fr.sun_dir_model))       # (both rasters are 16:9: one camera)
    ctx.upload(scene)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream()
    raw = stream.cuda_stream
    cats = {}
    for n in COUNTS:
        ra, dec, mag = d.synthetic_star_catalog(11, n, 0.0, 9.0)
        world, flux = d.stars_from_catalog(ra, dec, mag, (50.0, 50.0, 50.0))
        cats[n] = (torch.from_numpy(d.pose_to_model(pose, world, direction=True)).to(dev), torch.from_numpy(flux).to(dev))
    out = {"reps": a.reps, "sizes": {}}
    for W, H in SIZES:
        desc = d.make_desc(W, H, 1)
        lin = torch.rand((H, W, 3), dtype=torch.float32, device=dev)
        frame_out = torch.empty_like(lin)
        row = {}
        for n in COUNTS:
            dirs, flux = cats[n]
            first = ctx.render_stars(desc, dirs, flux, linear=lin, want=("layer", "status"))
            torch.cuda.synchronize()
            status = first["status"]
            window = (status & 1) != 0
            in_dirs = dirs[window].contiguous()
            origin = torch.tensor([scene.camera.origin.x, scene.camera.origin.y, scene.camera.origin.z], dtype=torch.float32, device=dev)
            in_orig = origin.expand(in_dirs.shape[0], 3).contiguous()
            layer = first["layer"]
            xy = torch.empty((n, 2), dtype=torch.float32, device=dev)
            st = torch.empty((n,), dtype=torch.uint8, device=dev)
            blocked = torch.empty((in_dirs.shape[0],), dtype=torch.uint8, device=dev)

            def stars(count, occlusion, image):
                s = d.capi.DsrtStars(count, occlusion, dirs.data_ptr(), flux.data_ptr(), lin.data_ptr())
                o = d.capi.DsrtStarsOut(None, frame_out.data_ptr() if image else None, xy.data_ptr(), st.data_ptr())
                rc = d.lib.dsrt_render_stars(ctx._h, desc, s, o, raw, None)
                assert rc == 0, d.lib.dsrt_last_error()

            def trace():
                rays = d.capi.DsrtRays(origins=in_orig.data_ptr(), dirs=in_dirs.data_ptr())
                hits = d.capi.DsrtRayHits(flags=blocked.data_ptr())
                rc = d.lib.dsrt_trace_rays(ctx._h, int(in_dirs.shape[0]), rays, d.capi.TRACE_ANY, hits, raw, None)
                assert rc == 0, d.lib.dsrt_last_error()

            def add():
                torch.add(lin, layer, out=frame_out)

            cfgs = {"stars": lambda: stars(n, 1, True), "labels": lambda: stars(n, 1, False), "no_occlusion": lambda: stars(n, 0, True), "empty": lambda: stars(0, 1, True),
                    "composition": lambda: (trace(), add()), "composition_trace": trace, "composition_add": add}
            names = list(cfgs)
            ms = {}
            for rep in range(a.warmup + a.reps):
                k = rep % len(names)
                for cfg in names[k:] + names[:k]:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    cfgs[cfg]()
                    e1.record(stream)
                    e1.synchronize()
                    if rep >= a.warmup:
                        ms.setdefault(cfg, []).append(e0.elapsed_time(e1))
            med = {k: statistics.median(v) for k, v in ms.items()}
            vis = int(((status & 2) != 0).sum())
            row[str(n)] = {"in_window": int(window.sum()), "visible": vis, "median_ms": med, "min_ms": {k: min(v) for k, v in ms.items()},
                           "max_ms": {k: max(v) for k, v in ms.items()}, "spread_ms": {k: max(v) - min(v) for k, v in ms.items()},
                           "phases_ms": {"resolve": med["empty"], "walk": med["stars"] - med["no_occlusion"], "project_and_deposit": med["no_occlusion"] - med["empty"]},
                           "stars_over_composition": med["stars"] / med["composition"]}
            say(f"{W}x{H}, {n} stars: timed")
        out["sizes"][f"{W}x{H}"] = row
    ctx.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
