#!/usr/bin/env python3
"""Measurement (not a test): the G-buffer pass (include/dsrt.h, dsrt_render_gbuffer) on the bench's scene -- the 1,000,000-triangle stand-in
mesh, pose frame 98, 1920x1080 -- timed with HIP events over `--reps` launches after a warm-up, for (a) every channel and (b) t + prim_id + flags
only; three full rows of (a) are checked against the CPU oracle bit for bit.  Prints one JSON line.

usage: tools/gbuffer_probe.py [--tris 1000000] [--frame 98] [--reps 50]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tris", type=int, default=1000000)
    ap.add_argument("--frame", type=int, default=98)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import torch
    import dsrt_amd as d
    from dsrt_amd import capi, meshgen
    from conftest import Oracle
    from test_gpu_gbuffer import assert_same, expected_gbuffer
    obj = f"/tmp/dsrt_bench_station_v{meshgen.VERSION}_{a.tris}.obj"
    if not os.path.exists(obj):
        tmp = obj + f".{os.getpid()}.tmp"
        meshgen.write_obj(meshgen.build_station(a.tris), tmp, mtl_name=os.path.basename(obj)[:-4] + ".mtl")
        os.replace(tmp, obj)
    hs = d.HostScene().add_obj(obj)
    hs.build_bvh()
    fr = d.pose_to_frame(d.read_pose_file(os.path.join(ROOT, "tests", "golden", "rendezvous_1s_dt0_01s.txt"))[a.frame])
    W, H = a.width, a.height
    scene = hs.view(d.frame_camera(fr, 40.0, W, H, 1, 50), tuple(fr.sun_dir_model))
    ctx = d.Context(0)
    ctx.upload(scene)
    desc = d.make_desc(W, H, 1)
    torch_dt = {"<f4": torch.float32, "<i4": torch.int32, "u1": torch.uint8}
    bufs = {n: torch.zeros((H, W, c) if c > 1 else (H, W), dtype=torch_dt[dt], device="cuda") for n, (dt, c) in capi.GBUFFER_CHANNELS.items()}
    stream = torch.cuda.current_stream()
    result = {"scene": f"station {a.tris} triangles, pose frame {a.frame}", "width": W, "height": H, "reps": a.reps}
    for label, names in (("all_channels", list(bufs)), ("t_prim_flags", ["t", "prim_id", "flags"])):
        ptrs = {n: bufs[n].data_ptr() for n in names}
        for _ in range(a.warmup):
            ctx.render_gbuffer(desc, ptrs, stream=stream.cuda_stream)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(a.reps):
            ctx.render_gbuffer(desc, ptrs, stream=stream.cuda_stream)
        e1.record(stream)
        e1.synchronize()
        ms = e0.elapsed_time(e1) / a.reps
        st = ctx.render_gbuffer(desc, ptrs, stream=stream.cuda_stream, want_stats=True)
        flags = bufs["flags"].cpu().numpy()
        result[label] = {"ms_per_launch": round(ms, 4), "primary_rays_per_s": W * H / (ms * 1e-3), "single_launch_kernel_ms": round(st.kernel_ms, 4),
                         "hit_fraction": float((flags & 1).mean()), "sunlit_fraction": float(((flags & 8) != 0).mean())}
    # every channel once more, and three full rows of it against the oracle
    ctx.render_gbuffer(desc, {k: b.data_ptr() for k, b in bufs.items()}, stream=stream.cuda_stream)
    torch.cuda.synchronize()
    got = {n: b.cpu().numpy() for n, b in bufs.items()}
    rows = [H // 2, H // 8, H - 1 - H // 10]
    want = expected_gbuffer(Oracle(), hs, scene, W, H, rows=rows)
    assert_same(got, want, rows=rows)
    result["oracle_rows_checked"] = rows
    result["oracle_rows_bit_identical"] = True
    ctx.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
