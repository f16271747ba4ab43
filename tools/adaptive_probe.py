#!/usr/bin/env python3
"""Measurement (not a test): what adaptive sampling costs and saves (include/dsrt.h, ADAPTIVE SAMPLING) on the bench's frame -- the 1,000,000-triangle
stand-in mesh, pose frame 98, 1920x1080 planned at 1000 spp, rng_mode 1, rays on the certified second tree.  Every figure is HIP-event time on one stream
around the whole operation (pre-pass, list building, render kernel, and for the driver its tests, readbacks and resolve), after a warm-up, settings
interleaved rep by rep, medians.  Every comparison is made inside one run:
  (a) render, acc         dsrt_render and one unmasked dsrt_render_accumulate of [0, 1000); with --base-root (a checkout of the parent commit, its library
                          built) the same two of that library, in child processes that alternate with this library's -- the probe's own spread
  (b) pass, ones, empty   an unmasked pass of 250 samples (first 0, stride 4), the same pass masked with all ones, and with an all-zero mask (pre-pass, the
                          list-building kernels on a mask without work for them, a render kernel that finds two empty lists: what a masked launch costs at
                          least); and list_kernels_us: the three list-building kernels of the all-ones pass on their own, from a kernel trace (rocprofv3
                          --kernel-trace --stats around a child of its own that runs only such passes; skipped with --no-trace)
  (c) rnd_F, clu_F        the masked pass at F = 0.5, 0.1, 0.01 of the pixels that see geometry, chosen at random and clustered (whole tiles in raster order)
  (d) adaptive_T          dsrt_render_adaptive at three tolerances, P = 8, min_passes = 2: time, samples_total / (W*H*spp), RMSE of the float image against a
                          1000-spp image of another seed; and fixed_T: dsrt_render at the spp that takes about the same time, with its RMSE
Prints one JSON line per child and a summary line.

usage: tools/adaptive_probe.py [--base-root DIR] [--no-trace] [--rounds 2] [--reps 3] [--warmup 1] [--tols 0.02,0.05,0.1] [--tris 1000000] [--frame 98]
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRACTIONS = (0.5, 0.1, 0.01)


def child(a):
    sys.path.insert(0, a.root)
    import numpy as np
    import torch
    import dsrt_amd as d
    from dsrt_amd import meshgen
    obj = f"/tmp/dsrt_bench_station_v{meshgen.VERSION}_{a.tris}.obj"
    if not os.path.exists(obj):
        tmp = obj + f".{os.getpid()}.tmp"
        meshgen.write_obj(meshgen.build_station(a.tris), tmp, mtl_name=os.path.basename(obj)[:-4] + ".mtl")
        os.replace(tmp, obj)
    W, H, spp, depth = a.width, a.height, a.spp, 50
    hs = d.HostScene().add_obj(obj)
    hs.build_bvh()
    fr = d.pose_to_frame(d.read_pose_file(os.path.join(ROOT, "tests", "golden", "rendezvous_1s_dt0_01s.txt"))[a.frame])
    scene = hs.view(d.frame_camera(fr, 40.0, W, H, spp, depth), tuple(fr.sun_dir_model))
    ctx = d.Context(0).set_certified_tree(True)
    ctx.upload(scene)
    desc = d.make_desc(W, H, spp, depth, rng_mode=1)
    stream = torch.cuda.current_stream()
    raw = stream.cuda_stream
    dev = "cuda:0"
    rgb = torch.empty(W * H * 3, dtype=torch.uint8, device=dev)
    f32 = torch.empty(W * H * 3, dtype=torch.float32, device=dev)
    sums = torch.zeros(W * H * 3, dtype=torch.int64, device=dev)
    sq = torch.zeros(W * H * 3, dtype=torch.int64, device=dev)
    base = a.child == "base"
    tols = [float(t) for t in a.tols.split(",")]
    P, M = 8, 2
    pass_set = (0, len(range(0, spp, 4)), 4)

    masks, out = {}, {"child": a.child}
    if a.child == "trace":                   # under the kernel trace: all-ones masked passes and nothing else
        ones = torch.ones(W * H, dtype=torch.uint8, device=dev)
        for _ in range(a.warmup + a.reps):
            ctx.render_accumulate_masked(desc, *pass_set, sums=sums, mask=ones, stream=raw)
        torch.cuda.synchronize()
        print(json.dumps(out), flush=True)
        return
    if not base:
        # the pixels that see geometry: nonzero sums of one unmasked pass
        ctx.render_accumulate(desc, *pass_set, sums=sums, stream=raw)
        torch.cuda.synchronize()
        hit = (sums.view(H, W, 3).max(dim=2).values > 0).cpu().numpy()
        out["hit_fraction"] = float(hit.mean())
        masks["ones"] = np.ones((H, W), np.uint8)
        masks["empty"] = np.zeros((H, W), np.uint8)
        rng = np.random.default_rng(1)
        ys, xs = np.nonzero(hit)
        tile_order = np.argsort((ys // 8) * ((W + 7) // 8) + xs // 8, kind="stable")
        for f in FRACTIONS:
            k = max(1, int(round(f * len(ys))))
            pick = rng.choice(len(ys), size=k, replace=False)
            m = np.zeros((H, W), np.uint8); m[ys[pick], xs[pick]] = 1
            masks[f"rnd_{f}"] = m
            m = np.zeros((H, W), np.uint8); m[ys[tile_order[:k]], xs[tile_order[:k]]] = 1
            masks[f"clu_{f}"] = m
        masks = {k: torch.from_numpy(v).to(dev) for k, v in masks.items()}
        # the yardstick of (d): the frame at full spp with another seed
        other = d.make_desc(W, H, spp, depth, rng_mode=1, seed=desc.seed + 7919)
        ref = torch.empty(W * H * 3, dtype=torch.float32, device=dev)
        ctx.render(other, rgb.data_ptr(), ref.data_ptr(), stream=raw)
        torch.cuda.synchronize()
    configs = ["render", "acc"] + ([] if base else ["pass"] + list(masks) + [f"adaptive_{t}" for t in tols])
    extra = {}

    def rmse(img):
        return float(torch.sqrt(torch.mean((img.reshape(-1).double() - ref.double()) ** 2)))

    def run(cfg):
        if cfg == "render":
            ctx.render(desc, rgb.data_ptr(), stream=raw)
        elif cfg.startswith("fixed_"):
            ctx.render(extra[cfg], rgb.data_ptr(), f32.data_ptr(), stream=raw)
        elif cfg == "acc":
            sums.zero_()
            ctx.render_accumulate(desc, 0, spp, 1, sums=sums, stream=raw)
        elif cfg == "pass":
            ctx.render_accumulate(desc, *pass_set, sums=sums, stream=raw)
        elif cfg in masks:
            ctx.render_accumulate_masked(desc, *pass_set, sums=sums, mask=masks[cfg], stream=raw)
        else:
            tol = float(cfg.split("_")[1])
            acc, (_, img, _), st = ctx.render_adaptive(desc, tol, passes=P, min_passes=M, want_rgb8=False, want_f32=True, stream=raw)
            extra[cfg] = (st, img)

    ms = {}

    def measure(cfgs):
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

    measure(configs)
    med = {c: statistics.median(v) for c, v in ms.items()}
    if not base:
        # (d): what the adaptive frames are worth, and fixed-spp renders of about the same time
        rows, fixed = {}, []
        for t in tols:
            st, img = extra[f"adaptive_{t}"]
            rows[str(t)] = {"ms": med[f"adaptive_{t}"], "sample_fraction": st["samples_total"] / (W * H * spp), "passes_run": st["passes_run"],
                            "active": st["active"], "rmse": rmse(img)}
            k = max(2, min(spp, int(round(spp * med[f"adaptive_{t}"] / med["render"]))))
            extra[f"fixed_{t}"] = d.make_desc(W, H, k, depth, rng_mode=1)
            rows[str(t)]["fixed_spp"] = k
            fixed.append(f"fixed_{t}")
        measure(fixed)
        for t in tols:
            run(f"fixed_{t}")
            torch.cuda.synchronize()
            rows[str(t)]["fixed_ms"] = statistics.median(ms[f"fixed_{t}"])
            rows[str(t)]["fixed_rmse"] = rmse(f32)
        ctx.render(desc, rgb.data_ptr(), f32.data_ptr(), stream=raw)
        torch.cuda.synchronize()
        out["rmse_full_spp"] = rmse(f32)
        out["adaptive"] = rows
        med = {c: statistics.median(v) for c, v in ms.items()}
    out["ms"] = ms
    out["median_ms"] = med
    print(json.dumps(out), flush=True)


def trace_list_kernels(script, common):
    """Average duration (us) of every list-building kernel over the all-ones passes of a traced child, by kernel name."""
    if not shutil.which("rocprofv3"):
        return {"error": "rocprofv3 not found"}
    with tempfile.TemporaryDirectory() as tmp:
        out = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, script, "--child", "trace"] + common,
                             capture_output=True, text=True, timeout=600)
        if out.returncode != 0:
            return {"error": (out.stdout[-500:] + out.stderr[-1500:])}
        res = {}
        for f in glob.glob(tmp + "/**/*kernel_stats.csv", recursive=True):
            for r in csv.DictReader(open(f)):
                if "dsrt_pixel_" in r["Name"]:
                    res[r["Name"].split("(")[0]] = {"calls": int(r["Calls"]), "avg_us": float(r["AverageNs"]) / 1e3}
        return res or {"error": "no list-building kernel in the trace"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=["base", "new", "trace"])
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--base-root")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--tols", default="0.02,0.05,0.1")
    ap.add_argument("--tris", type=int, default=1000000)
    ap.add_argument("--frame", type=int, default=98)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=1000)
    a = ap.parse_args()
    if a.child:
        return child(a)
    common = ["--reps", str(a.reps), "--warmup", str(a.warmup), "--tols", a.tols, "--tris", str(a.tris), "--frame", str(a.frame), "--width", str(a.width),
              "--height", str(a.height), "--spp", str(a.spp)]
    runs = [("new", ROOT)] + ([("base", os.path.abspath(a.base_root))] if a.base_root else [])
    med, last = {}, None
    for r in range(a.rounds):
        for kind, root in (runs if r % 2 == 0 else runs[::-1]):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", kind, "--root", root] + common, capture_output=True, text=True, timeout=1100)
            if out.returncode != 0:
                print(out.stdout[-2000:] + out.stderr[-4000:], file=sys.stderr)
                raise SystemExit(out.returncode)
            line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
            print(line, flush=True)
            rec = json.loads(line)
            if kind == "new":
                last = rec
            for c, v in rec["median_ms"].items():
                med.setdefault(f"{kind}:{c}", []).append(v)
    m = {k: statistics.median(v) for k, v in med.items()}
    summary = {"median_ms": m, "per_round": {k: v for k, v in med.items() if k.split(":")[1] in ("render", "acc")},
               "b_ones_vs_pass_ms": m["new:ones"] - m["new:pass"], "b_empty_mask_launch_ms": m["new:empty"],
               "c_fraction_of_pass": {k.split(":")[1]: m[k] / m["new:pass"] for k in m if k.startswith("new:rnd_") or k.startswith("new:clu_")},
               "d_adaptive": last["adaptive"], "hit_fraction": last["hit_fraction"], "rmse_full_spp": last["rmse_full_spp"]}
    if not a.no_trace:
        summary["b_list_kernels_us"] = trace_list_kernels(os.path.abspath(__file__), ["--root", ROOT] + common)
    if "base:render" in m:
        summary["a_render_new_vs_base"] = m["new:render"] / m["base:render"]
        summary["a_acc_new_vs_base"] = m["new:acc"] / m["base:acc"]
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
