#!/usr/bin/env python3
"""Measurement (not a test): the coverage pass (include/dsrt.h, COVERAGE: dsrt_render_coverage) on the bench's scene -- the 1,000,000-triangle stand-in mesh,
pose frame 98, 1920x1080 -- timed with HIP events after a warm-up: GRID 2, 4, 8 and DIAGONAL 16, 64, each with the sun outputs (hits, alpha, mask and their sun
forms: shadow rays traced) and without (hits, alpha, mask), against the yardstick of n G-buffer launches timed in the same process (t + flags with the shadow
rays, t alone without): the coverage pass traces the same number of rays, and more coherent ones.  Then the coverage-aware denoise call against
dsrt_denoise_accumulated on one frame of that scene.  Prints one JSON line.

usage: tools/coverage_probe.py [--tris 1000000] [--frame 98] [--reps 20] [--spp 16]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tris", type=int, default=1000000)
    ap.add_argument("--frame", type=int, default=98)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--spp", type=int, default=16)
    a = ap.parse_args()
    import torch
    import dsrt_amd as d
    from dsrt_amd import meshgen
    obj = f"/tmp/dsrt_bench_station_v{meshgen.VERSION}_{a.tris}.obj"
    if not os.path.exists(obj):
        tmp = obj + f".{os.getpid()}.tmp"
        meshgen.write_obj(meshgen.build_station(a.tris), tmp, mtl_name=os.path.basename(obj)[:-4] + ".mtl")
        os.replace(tmp, obj)
    hs = d.HostScene().add_obj(obj)
    hs.build_bvh()
    fr = d.pose_to_frame(d.read_pose_file(os.path.join(ROOT, "tests", "golden", "rendezvous_1s_dt0_01s.txt"))[a.frame])
    W, H = a.width, a.height
    scene = hs.view(d.frame_camera(fr, 40.0, W, H, a.spp, 50), tuple(fr.sun_dir_model))
    ctx = d.Context(0)
    ctx.upload(scene)
    desc = d.make_desc(W, H, a.spp, rng_mode=1)
    stream = torch.cuda.current_stream()
    raw = stream.cuda_stream

    def timed(call, reps):
        for _ in range(a.warmup):
            call()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(reps):
            call()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    def buf(dtype, *tail):
        return torch.zeros((H, W) + tail, dtype=dtype, device="cuda")

    result = {"scene": f"station {a.tris} triangles, pose frame {a.frame}", "width": W, "height": H, "reps": a.reps}
    t, flags = buf(torch.float32), buf(torch.uint8)
    gb_sun = timed(lambda: ctx.render_gbuffer(desc, {"t": t.data_ptr(), "flags": flags.data_ptr()}, stream=raw), a.reps)
    gb_plain = timed(lambda: ctx.render_gbuffer(desc, {"t": t.data_ptr()}, stream=raw), a.reps)
    result["gbuffer"] = {"t_flags_ms": round(gb_sun, 4), "t_ms": round(gb_plain, 4), "hit_fraction": float((flags & 1).float().mean())}
    own = {"hits": buf(torch.uint8), "alpha": buf(torch.float32), "mask": buf(torch.int64)}
    sun = {"sun_hits": buf(torch.uint8), "sun_alpha": buf(torch.float32), "sun_mask": buf(torch.int64)}
    result["coverage"] = {}
    for pattern, samples in (("grid", 2), ("grid", 4), ("grid", 8), ("diag", 16), ("diag", 64)):
        cd = d.coverage_desc(pattern, samples)
        n = samples * samples if pattern == "grid" else samples
        reps = max(3, a.reps // max(1, n // 4))
        with_sun = timed(lambda: ctx.render_coverage(desc, cd, {k: x.data_ptr() for k, x in {**own, **sun}.items()}, stream=raw), reps)
        partial = float(((own["hits"] > 0) & (own["hits"] < n)).float().mean())
        without = timed(lambda: ctx.render_coverage(desc, cd, {k: x.data_ptr() for k, x in own.items()}, stream=raw), reps)
        result["coverage"][f"{pattern}:{samples}"] = {
            "n": n, "reps": reps, "sun_ms": round(with_sun, 4), "no_sun_ms": round(without, 4), "rays_per_s_no_sun": W * H * n / (without * 1e-3),
            "ratio_to_n_gbuffer_launches_sun": round(with_sun / (n * gb_sun), 4), "ratio_to_n_gbuffer_launches_no_sun": round(without / (n * gb_plain), 4),
            "partially_covered_fraction": partial}
    # the coverage-aware denoise call against the plain one, on one frame's sums
    acc = d.Accumulator(ctx, desc, moments=True)
    acc.render(0)
    guides = acc.guides()
    alpha, rep = acc.coverage()
    torch.cuda.synchronize()
    plain = timed(lambda: ctx.denoise_accumulated(desc, acc.sum, acc.sum_sq, guides, samples_done=a.spp, want_var=True), a.reps)
    aware_same_guides = timed(lambda: ctx.denoise_accumulated_coverage(desc, acc.sum, acc.sum_sq, guides, alpha, samples_done=a.spp, want_var=True), a.reps)
    aware = timed(lambda: ctx.denoise_accumulated_coverage(desc, acc.sum, acc.sum_sq, rep, alpha, samples_done=a.spp, want_var=True), a.reps)
    result["denoise"] = {"spp": a.spp, "plain_ms": round(plain, 4), "coverage_aware_same_guides_ms": round(aware_same_guides, 4), "coverage_aware_rep_guides_ms": round(aware, 4),
                         "ratio_same_guides": round(aware_same_guides / plain, 4), "ratio_rep_guides": round(aware / plain, 4),
                         "note": "timed calls include the output allocations of the Python wrapper, the same in all three"}
    ctx.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
