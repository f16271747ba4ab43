#!/usr/bin/env python3
"""Measurement (not a test): what the G-buffer-guided upscaler costs (include/dsrt.h, UPSCALER) on the bench's scene -- the 1,000,000-triangle stand-in mesh, pose
frame 98, rng_mode 1, rays on the certified second tree -- at 960x540 -> 1920x1080 and 1920x1080 -> 3840x2160.  Device times are HIP-event times on one stream
around the operation, `--reps` launches after `--warmup`, configurations interleaved rep by rep, medians; the whole-frame figures are host wall times around
synchronous _to_host calls (`--frame-reps` of them), result copies included.  Per size pair:
  upscale_call        dsrt_upscale_guided (its two launches: pack + the upscale kernel) writing rgb8 and linear
  gbuffer_hi          dsrt_render_gbuffer of the five guide channels at the output size
  atrous_iteration    the yardstick: one a-trous iteration of the denoiser at the OUTPUT size (two iterations minus one, same run, the denoiser's unchanged kernel)
  frame_upscaled_64   dsrt_render_upscaled_to_host: 64 spp at the low resolution, denoised (defaults), upscaled
  frame_native_64/16  dsrt_render_denoised_to_host at the output size with 64 and with 16 spp
  upscale_coverage_call   dsrt_upscale_guided_coverage (include/dsrt.h, COVERAGE-AWARE UPSCALER) on the alphas and representatives of DIAGONAL 64 coverage passes at both
                      rasters and the coverage-denoised low-resolution frame, interleaved with upscale_call in the same process; covered_fraction (alpha > 0 at the
                      output raster) and the pixels per level say how many more pixels do work than hit_fraction's
  coverage_hi_8/16/64 dsrt_render_coverage (alpha and the five representative channels) at the output size, DIAGONAL 8, 16 and 64: what the form adds to a frame
  frame_upscaled_coverage_64_n8/16/64   dsrt_render_upscaled_coverage_to_host: 64 spp at the low resolution, both coverage passes DIAGONAL n, coverage-denoised, upscaled
  kernels_us          with --trace: every upscale / a-trous kernel's average from a kernel trace (rocprofv3 --kernel-trace --stats around a child of its own that runs
                      only upscale calls and two-iteration denoise calls): the upscale kernel's time ALONE
Prints one JSON line.

usage: tools/upscale_probe.py [--trace] [--reps 20] [--warmup 3] [--frame-reps 5] [--tris 1000000] [--frame 98] [--spp 64]
"""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = ((960, 540, 1920, 1080), (1920, 1080, 3840, 2160))
CHANNELS = {"normal": 3, "position": 3, "albedo": 3, "range": 1, "flags": 1}


def child(a):
    sys.path.insert(0, ROOT)
    import torch
    import dsrt_amd as d
    from dsrt_amd import meshgen
    obj = f"/tmp/dsrt_bench_station_v{meshgen.VERSION}_{a.tris}.obj"
    if not os.path.exists(obj):
        tmp = obj + f".{os.getpid()}.tmp"
        meshgen.write_obj(meshgen.build_station(a.tris), tmp, mtl_name=os.path.basename(obj)[:-4] + ".mtl")
        os.replace(tmp, obj)
    depth = 50
    say = lambda what: print(f"[upscale_probe {a.child}] {what}", file=sys.stderr, flush=True)   # noqa: E731
    say("mesh written")
    hs = d.HostScene().add_obj(obj)
    hs.build_bvh()
    say("scene built")
    fr = d.pose_to_frame(d.read_pose_file(os.path.join(ROOT, "tests", "golden", "rendezvous_1s_dt0_01s.txt"))[a.frame])
    ctx = d.Context(0).set_certified_tree(True)
    ctx.upload(hs.view(d.frame_camera(fr, 40.0, PAIRS[0][2], PAIRS[0][3], a.spp, depth), tuple(fr.sun_dir_model)))     # (every raster here is 16:9: one camera)
    stream = torch.cuda.current_stream()
    raw = stream.cuda_stream
    dev = "cuda:0"
    out = {"child": a.child, "spp": a.spp, "reps": a.reps, "frame_reps": a.frame_reps, "pairs": {}}

    def gbuffer(desc, g=None):
        if g is None:
            g = {k: torch.empty((desc.height, desc.width, n) if n == 3 else (desc.height, desc.width), dtype=torch.uint8 if k == "flags" else torch.float32, device=dev)
                 for k, n in CHANNELS.items()}
        ctx.render_gbuffer(desc, {k: x.data_ptr() for k, x in g.items()}, stream=raw)
        return g

    for (w, h, W, H) in PAIRS:
        lo_desc, hi_desc = d.make_desc(w, h, a.spp, depth, rng_mode=1), d.make_desc(W, H, a.spp, depth, rng_mode=1)
        acc = d.Accumulator(ctx, lo_desc, moments=True)
        acc.render(0, stream=raw)
        lo = gbuffer(lo_desc)
        four = lambda g: {k: g[k] for k in d.DENOISE_GUIDES}                          # noqa: E731
        _, _, c, v = ctx.denoise_accumulated(lo_desc, acc.sum, acc.sum_sq, four(lo), samples_done=a.spp, want_rgb8=False, want_var=True, stream=raw)
        hi = gbuffer(hi_desc)
        cov = {n: d.coverage_desc("diag", n) for n in (8, 16, 64)}

        def coverage(desc, n, alpha=None, g=None):
            if g is None:
                alpha = torch.empty((desc.height, desc.width), dtype=torch.float32, device=dev)
                g = gbuffer(desc)
            ctx.render_coverage(desc, cov[n], {"alpha": alpha.data_ptr()}, {k: x.data_ptr() for k, x in g.items()}, stream=raw)
            return alpha, g

        a_lo, r_lo = coverage(lo_desc, 64)
        _, _, cc, cv = ctx.denoise_accumulated_coverage(lo_desc, acc.sum, acc.sum_sq, four(r_lo), a_lo, samples_done=a.spp, want_rgb8=False, want_var=True, stream=raw)
        a_hi, r_hi = coverage(hi_desc, 64)
        few = d.make_desc(W, H, 2, depth, rng_mode=1)                                # the yardstick's frame: sums at the output size (two samples: only the filter is timed)
        acc_hi = d.Accumulator(ctx, few, moments=True)
        acc_hi.render(0, stream=raw)
        torch.cuda.synchronize()
        say(f"{w}x{h} -> {W}x{H}: inputs rendered")

        def run(cfg):
            if cfg == "upscale_call":
                ctx.upscale_guided(hi_desc, w, h, c, lo, hi, lo_var=v, stream=raw)
            elif cfg == "upscale_coverage_call":
                ctx.upscale_guided_coverage(hi_desc, w, h, cc, r_lo, r_hi, a_lo, a_hi, lo_var=cv, stream=raw)
            elif cfg == "gbuffer_hi":
                gbuffer(hi_desc, hi)
            elif cfg.startswith("coverage_hi_"):
                coverage(hi_desc, int(cfg.rsplit("_", 1)[1]), a_tmp, r_tmp)
            else:
                ctx.denoise_accumulated(few, acc_hi.sum, acc_hi.sum_sq, four(hi), samples_done=2, params=d.denoise_defaults(iterations=int(cfg[-1])), stream=raw)

        a_tmp, r_tmp = coverage(hi_desc, 8)                                          # (the timed coverage passes write here: a_hi / r_hi stay DIAGONAL 64's)
        cfgs = ["upscale_call", "upscale_coverage_call", "atrous_1", "atrous_2"] + ([] if a.child == "trace" else ["gbuffer_hi", "coverage_hi_8", "coverage_hi_16", "coverage_hi_64"])
        ms = {}
        for rep in range(a.warmup + a.reps):
            k = rep % len(cfgs)
            for cfg in cfgs[k:] + cfgs[:k]:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                run(cfg)
                e1.record(stream)
                e1.synchronize()
                if rep >= a.warmup:
                    ms.setdefault(cfg, []).append(e0.elapsed_time(e1))
        med = {k: statistics.median(x) for k, x in ms.items()}
        say(f"{w}x{h} -> {W}x{H}: launches timed")
        row = {"median_ms": med, "min_ms": {k: min(x) for k, x in ms.items()}, "max_ms": {k: max(x) for k, x in ms.items()},
               "atrous_iteration_ms": med["atrous_2"] - med["atrous_1"], "hit_fraction": float(torch.isfinite(hi["range"]).double().mean())}
        row["upscale_call_over_iteration"] = med["upscale_call"] / row["atrous_iteration_ms"]
        row["upscale_coverage_call_over_upscale_call"] = med["upscale_coverage_call"] / med["upscale_call"]
        row["covered_fraction"] = float((a_hi > 0).double().mean())
        level = ctx.upscale_guided_coverage(hi_desc, w, h, cc, r_lo, r_hi, a_lo, a_hi, want_rgb8=False, want_linear=False, want_level=True, stream=raw)[5]
        row["pixels_per_level"] = torch.bincount(level.flatten().long(), minlength=4).tolist()
        if a.child != "trace":
            frames = {"frame_upscaled_64": lambda: ctx.render_upscaled_to_host(lo_desc, W, H, denoise=d.denoise_defaults()),
                      **{f"frame_upscaled_coverage_64_n{n}": (lambda n=n: ctx.render_upscaled_coverage_to_host(lo_desc, W, H, cov_lo=cov[n], cov_hi=cov[n],
                                                                                                                   denoise=d.denoise_defaults())) for n in (8, 16, 64)},
                      "frame_native_coverage_64": lambda: ctx.render_denoised_coverage_to_host(hi_desc),
                      "frame_native_coverage_16": lambda: ctx.render_denoised_coverage_to_host(d.make_desc(W, H, max(a.spp // 4, 2), depth, rng_mode=1)),
                      "frame_native_64": lambda: ctx.render_denoised_to_host(hi_desc),
                      "frame_native_16": lambda: ctx.render_denoised_to_host(d.make_desc(W, H, max(a.spp // 4, 2), depth, rng_mode=1))}
            wall = {}
            for rep in range(1 + a.frame_reps):
                for name, fn in frames.items():
                    t0 = time.perf_counter()
                    fn()
                    if rep:
                        wall.setdefault(name, []).append((time.perf_counter() - t0) * 1e3)
            row["frame_wall_ms"] = {k: statistics.median(x) for k, x in wall.items()}
        out["pairs"][f"{w}x{h}->{W}x{H}"] = row
    print(json.dumps(out), flush=True)


def trace_kernels(script, common):
    """Average duration (us) of the upscale and a-trous kernels over a traced child's calls, by kernel name (both size pairs together are of no use: the
    child is run once per pair)."""
    if not shutil.which("rocprofv3"):
        return {"error": "rocprofv3 not found"}
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        run = subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "--", sys.executable, script, "--child", "trace"] + common,
                             stdout=subprocess.PIPE, text=True, timeout=1100)
        if run.returncode != 0:
            return {"error": run.stdout[-2000:]}
        for f in glob.glob(tmp + "/**/*kernel_trace.csv", recursive=True):
            for r in csv.DictReader(open(f)):
                name = r["Kernel_Name"].split("(")[0]
                if "dsrt_upscale" in name or "dsrt_denoise_atrous" in name:
                    grid = f"{r['Grid_Size_X']}x{r.get('Grid_Size_Y', '')}"                  # (the grid tells the size pairs apart)
                    res.setdefault(f"{name} grid {grid}", []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return {k: {"calls": len(x), "median_us": statistics.median(x)} for k, x in res.items()} or {"error": "no upscale kernel in the trace"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=["new", "trace"])
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frame-reps", type=int, default=5)
    ap.add_argument("--tris", type=int, default=1000000)
    ap.add_argument("--frame", type=int, default=98)
    ap.add_argument("--spp", type=int, default=64)
    a = ap.parse_args()
    if a.child:
        return child(a)
    common = ["--reps", str(a.reps), "--warmup", str(a.warmup), "--frame-reps", str(a.frame_reps), "--tris", str(a.tris), "--frame", str(a.frame), "--spp", str(a.spp)]
    run = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "new"] + common, stdout=subprocess.PIPE, text=True, timeout=1100)
    if run.returncode != 0:
        print(run.stdout[-2000:], file=sys.stderr)
        raise SystemExit(run.returncode)
    rec = json.loads([l for l in run.stdout.splitlines() if l.startswith("{")][-1])
    if a.trace:
        rec["kernels_us"] = trace_kernels(os.path.abspath(__file__), common)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
