#!/usr/bin/env python3
"""Measurement (not a test): what sample sets cost (include/dsrt.h, SAMPLE SETS) on the bench's frame -- the 1,000,000-triangle stand-in mesh, pose
frame 98, 1920x1080 x 1000 spp, rng_mode 1, rays on the certified second tree.  Every figure is HIP-event time on one stream around the whole operation
(pre-pass, render kernel, resolve, and the zeroing of the sums where there are sums), after a warm-up, with the settings interleaved rep by rep:
  render     dsrt_render (zeroes its own sums, renders, resolves)
  acc        one dsrt_render_accumulate of [0, 1000) into zeroed sums + dsrt_resolve_accumulated
  pass4      four interleaved passes (first = p, stride = 4), each followed by a resolve (a preview after every pass)
  pass10     the same with ten passes
  moments    `acc` with sum_sq (the MOMENTS kernel) and the variance of the mean resolved as well
With --base-root (a checkout of the commit before sample sets, its library built), `render` of that library is timed too, in child processes that
alternate with this library's: builds are only compared inside one run.  Prints one JSON line per child and a summary line of medians.

usage: tools/accum_probe.py [--base-root DIR] [--rounds 3] [--reps 4] [--warmup 2] [--tris 1000000] [--frame 98]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = ("render", "acc", "pass4", "pass10", "moments")


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
    rgb = torch.empty(W * H * 3, dtype=torch.uint8, device="cuda:0")
    n = W * H * 3
    sums = torch.zeros(n, dtype=torch.int64, device="cuda:0")
    sq = torch.zeros(n, dtype=torch.int64, device="cuda:0")
    configs = ("render",) if a.child == "base" else CONFIGS

    def run(cfg):
        if cfg == "render":
            ctx.render(desc, rgb.data_ptr(), stream=raw)
            return
        sums.zero_()
        with_sq = cfg == "moments"
        if with_sq:
            sq.zero_()
        passes = {"pass4": 4, "pass10": 10}.get(cfg, 1)
        done = 0
        for p in range(passes):
            count = len(range(p, spp, passes))
            ctx.render_accumulate(desc, p, count, passes, sums=sums, sum_sq=sq if with_sq else None, stream=raw)
            done += count
            ctx.resolve_accumulated(desc, sums, done, sum_sq=sq if with_sq else None, want_var=with_sq, stream=raw)

    ms = {c: [] for c in configs}
    for rep in range(a.warmup + a.reps):
        order = configs[rep % len(configs):] + configs[:rep % len(configs)]
        for cfg in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            run(cfg)
            e1.record(stream)
            e1.synchronize()
            if rep >= a.warmup:
                ms[cfg].append(e0.elapsed_time(e1))
    if a.child == "new":
        # the sets' union is the one-launch image: checked on the measured frame itself
        ctx.render(desc, rgb.data_ptr(), stream=raw)
        run("pass4")
        got, _, _ = ctx.resolve_accumulated(desc, sums, spp, stream=raw)
        torch.cuda.synchronize()
        assert torch.equal(got.reshape(-1), rgb), "four passes differ from the one-launch image"
    print(json.dumps({"child": a.child, "ms": ms, "median_ms": {c: statistics.median(v) for c, v in ms.items()}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=["base", "new"])
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--base-root")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tris", type=int, default=1000000)
    ap.add_argument("--frame", type=int, default=98)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=1000)
    a = ap.parse_args()
    if a.child:
        return child(a)
    common = ["--reps", str(a.reps), "--warmup", str(a.warmup), "--tris", str(a.tris), "--frame", str(a.frame), "--width", str(a.width),
              "--height", str(a.height), "--spp", str(a.spp)]
    runs = [("new", ROOT)] + ([("base", os.path.abspath(a.base_root))] if a.base_root else [])
    med = {}
    for r in range(a.rounds):
        for kind, root in (runs if r % 2 == 0 else runs[::-1]):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", kind, "--root", root] + common, capture_output=True, text=True, timeout=900)
            if out.returncode != 0:
                print(out.stdout[-2000:] + out.stderr[-4000:], file=sys.stderr)
                raise SystemExit(out.returncode)
            line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
            print(line, flush=True)
            for c, v in json.loads(line)["median_ms"].items():
                med.setdefault(f"{kind}:{c}", []).append(v)
    m = {k: statistics.median(v) for k, v in med.items()}
    summary = {"median_ms": m,
               "b_acc_vs_render": m["new:acc"] / m["new:render"],
               "c_pass4_vs_acc": m["new:pass4"] / m["new:acc"], "c_pass10_vs_acc": m["new:pass10"] / m["new:acc"],
               "d_moments_vs_acc": m["new:moments"] / m["new:acc"]}
    if "base:render" in m:
        summary["a_render_new_vs_base"] = m["new:render"] / m["base:render"]
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
