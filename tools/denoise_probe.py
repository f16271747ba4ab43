#!/usr/bin/env python3
"""Measurement (not a test): what the denoiser costs and buys (include/dsrt.h, DENOISER) on the bench's frame -- the 1,000,000-triangle stand-in mesh, pose
frame 98, 1920x1080, rng_mode 1, rays on the certified second tree.  Every time is HIP-event time on one stream around the whole operation, after a warm-up,
settings interleaved rep by rep, medians.  Every comparison is made inside one run:
  (a) render              dsrt_render at 1000 spp; with --base-root (a checkout of the parent commit, its library built) the same of that library, in child
                          processes that alternate with this library's -- the probe's own spread
  (b) denoise_I           dsrt_denoise_accumulated at I = 0 .. 5 iterations on the frame's sums and guides (I = 0: the prepare and the output kernel alone), the
                          nominal bytes of loads of an iteration, and floor_ms: what dsrt_microbench_copy takes for an iteration's compulsory bytes (every record
                          read once, the two that change written once); kernels_us: every kernel's average from a kernel trace (rocprofv3 --kernel-trace --stats
                          around a child of its own that runs only five-iteration calls; skipped with --no-trace)
  (c) rmse                of the LINEAR image against a 1000-spp image of another seed: raw at 1000 / 250 / 125 spp; denoised at 250 / 125 spp with the time of
                          the whole (accumulate with moments + G-buffer + denoise); and the fixed spp that takes about that time (dsrt_render's kernel through
                          dsrt_render_accumulate, which keeps the sums), with its RMSE
Prints one JSON line per child and a summary line.

usage: tools/denoise_probe.py [--base-root DIR] [--no-trace] [--rounds 2] [--reps 3] [--warmup 1] [--tris 1000000] [--frame 98]
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
RECORD = 16                                   # bytes of one of the filter's per-pixel records (csrc/launchers.h, DenoiseBuffers)


def child(a):
    sys.path.insert(0, a.root)
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
    out = {"child": a.child}
    low = [s for s in (spp // 4, spp // 8) if s >= 2]
    state, ms = {}, {}

    def accumulate(n, moments=True):
        acc = d.Accumulator(ctx, d.make_desc(W, H, n, depth, rng_mode=1), moments=moments)
        acc.render(0, stream=raw)
        return acc

    def linear(acc):
        return acc.sum.double() * (2.0 ** -20 / acc.samples_done)

    def run(cfg):
        if cfg == "render":
            ctx.render(desc, rgb.data_ptr(), stream=raw)
        elif cfg.startswith("denoise_"):
            acc, g = state["frame"]
            acc.denoise(params=d.denoise_defaults(iterations=int(cfg.split("_")[1])), guides=g, want_var=True, stream=raw)
        elif cfg.startswith("whole_"):
            acc = accumulate(int(cfg.split("_")[1]))
            state[cfg] = acc.denoise(want_rgb8=True, stream=raw)[2]
        elif cfg.startswith("fixed_"):
            state[cfg] = accumulate(int(cfg.split("_")[1]), moments=False)   # (dsrt_render's kernel, its sums kept for the linear image)

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

    if a.child == "base":
        measure(["render"])
    else:
        acc = accumulate(low[0])
        state["frame"] = (acc, acc.guides(stream=raw))
        torch.cuda.synchronize()
        out["hit_fraction"] = float(torch.isfinite(state["frame"][1]["range"]).double().mean())
        if a.child == "trace":                # under the kernel trace: five-iteration calls and nothing else
            for _ in range(a.warmup + a.reps):
                run("denoise_5")
            torch.cuda.synchronize()
            print(json.dumps(out), flush=True)
            return
        measure(["render"] + [f"denoise_{i}" for i in range(6)] + [f"whole_{s}" for s in low])
        med = {c: statistics.median(v) for c, v in ms.items()}
        # (b) the floor: an iteration reads five records per pixel once and writes two
        px = W * H
        moved = 7 * RECORD * px
        copy = d.microbench_copy(nbytes=moved // 2, reps=8)        # a copy of moved / 2 bytes reads and writes `moved` bytes
        out["iteration"] = {"load_bytes_per_filterable_pixel": 25 * 5 * RECORD + 9 * 4 + 3 * RECORD, "compulsory_bytes": moved,
                            "floor_ms": moved / (copy["GBps"] * 1e6), "copy_GBps": copy["GBps"], "working_set_bytes": 7 * RECORD * px}
        # (c) errors of the linear image against the full frame of another seed
        other = d.Accumulator(ctx, d.make_desc(W, H, spp, depth, rng_mode=1, seed=desc.seed + 7919))
        other.render(0, stream=raw)
        ref = linear(other)

        def rmse(img):
            return float(torch.sqrt(torch.mean((img.reshape(-1).double() - ref) ** 2)))

        rows = {"raw": {str(spp): rmse(linear(accumulate(spp, moments=False)))}, "denoised": {}}
        fixed = []
        for s in low:
            rows["raw"][str(s)] = rmse(linear(accumulate(s, moments=False)))
            k = max(2, min(spp, int(round(spp * med[f"whole_{s}"] / med["render"]))))
            rows["denoised"][str(s)] = {"ms": med[f"whole_{s}"], "rmse": rmse(state[f"whole_{s}"]), "fixed_spp": k}
            fixed.append(f"fixed_{k}")
        measure(fixed)
        for s, cfg in zip(low, fixed):
            rows["denoised"][str(s)]["fixed_ms"] = statistics.median(ms[cfg])
            rows["denoised"][str(s)]["fixed_rmse"] = rmse(linear(state[cfg]))
        out["rmse"] = rows
    out["ms"] = ms
    out["median_ms"] = {c: statistics.median(v) for c, v in ms.items()}
    print(json.dumps(out), flush=True)


def trace_kernels(script, common):
    """Average duration (us) of the filter's kernels over the five-iteration calls of a traced child, by kernel name."""
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
                if "dsrt_denoise_" in r["Name"]:
                    res[r["Name"].split("(")[0]] = {"calls": int(r["Calls"]), "avg_us": float(r["AverageNs"]) / 1e3}
        return res or {"error": "no denoise kernel in the trace"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=["base", "new", "trace"])
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--base-root")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--tris", type=int, default=1000000)
    ap.add_argument("--frame", type=int, default=98)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=1000)
    a = ap.parse_args()
    if a.child:
        return child(a)
    common = ["--reps", str(a.reps), "--warmup", str(a.warmup), "--tris", str(a.tris), "--frame", str(a.frame), "--width", str(a.width), "--height", str(a.height),
              "--spp", str(a.spp)]
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
    summary = {"median_ms": m, "per_round": {k: v for k, v in med.items() if k.split(":")[1] == "render"},
               "b_iteration_ms": {str(i): m[f"new:denoise_{i}"] - m[f"new:denoise_{i - 1}"] for i in range(1, 6)}, "b_prepare_and_output_ms": m["new:denoise_0"],
               "b_iteration": last["iteration"], "c_rmse": last["rmse"], "hit_fraction": last["hit_fraction"]}
    if not a.no_trace:
        summary["b_kernels_us"] = trace_kernels(os.path.abspath(__file__), ["--root", ROOT] + common)
    if "base:render" in m:
        summary["a_render_new_vs_base"] = m["new:render"] / m["base:render"]
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
