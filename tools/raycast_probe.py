#!/usr/bin/env python3
"""Measurement (not a test): the ray queries (include/dsrt.h, dsrt_trace_rays) on the bench's scene -- the 1,000,000-triangle stand-in mesh, pose
frame 98 -- timed with HIP events over `--reps` launches after a warm-up.  Prints one JSON line with rays/s for
  (a) the 1920x1080 pixel-centre rays through trace_rays (channels t + prim_id), next to dsrt_render_gbuffer with the same two channels;
  (b) 4 M incoherent rays: origins on a sphere of twice the scene's bounding radius, aimed at uniform points inside the root box (fixed seed);
  (c) the any-hit shadow rays of the frame's G-buffer hits (origin p + n * 1e-3, toward the Sun);
(a) is also compared with the G-buffer's answers, bit for bit.  (The lane-refill kernel this probe measured as (d) is not kept: DESIGN.md.)

usage: tools/raycast_probe.py [--tris 1000000] [--frame 98] [--reps 20]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tris", type=int, default=1000000)
    ap.add_argument("--frame", type=int, default=98)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--incoherent", type=int, default=4 << 20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
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
    scene = hs.view(d.frame_camera(fr, 40.0, W, H, 1, 50), tuple(fr.sun_dir_model))
    ctx = d.Context(0)
    ctx.upload(scene)
    stream = torch.cuda.current_stream()
    dev = torch.device("cuda", 0)

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(a.reps):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / a.reps

    # (a) pixel-centre rays, image order (top row first), as the G-buffer forms them: make_camera_ray_jittered with jx = jy = 0.5, in float32
    cam = scene.camera
    o = np.array([cam.origin.x, cam.origin.y, cam.origin.z], np.float32)
    llc = np.array([cam.lower_left_corner.x, cam.lower_left_corner.y, cam.lower_left_corner.z], np.float32)
    hor = np.array([cam.horizontal.x, cam.horizontal.y, cam.horizontal.z], np.float32)
    ver = np.array([cam.vertical.x, cam.vertical.y, cam.vertical.z], np.float32)
    xs = np.arange(W, dtype=np.float32)
    ky = (H - 1 - np.arange(H)).astype(np.float32)
    u = ((xs + np.float32(0.5)) / np.float32(W - 1))[None, :, None]
    v = ((ky + np.float32(0.5)) / np.float32(H - 1))[:, None, None]
    dirs = ((llc + hor * u) + ver * v) - o
    O_a = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(o, (H * W, 3)))).to(dev)
    D_a = torch.from_numpy(np.ascontiguousarray(dirs.reshape(-1, 3).astype(np.float32))).to(dev)
    gbuf = {"t": torch.empty((H, W), dtype=torch.float32, device=dev), "prim_id": torch.empty((H, W), dtype=torch.int32, device=dev)}
    desc = d.make_desc(W, H, 1)
    gptrs = {k: b.data_ptr() for k, b in gbuf.items()}
    result = {"scene": f"station {a.tris} triangles, pose frame {a.frame}", "reps": a.reps}
    ms = timed(lambda: ctx.render_gbuffer(desc, gptrs, stream=stream.cuda_stream))
    result["a_gbuffer_t_prim"] = {"rays": W * H, "ms": round(ms, 4), "rays_per_s": W * H / (ms * 1e-3)}

    def trace(O, D, **kw):
        return lambda: ctx.trace_rays(O, D, stream=stream, **kw)

    ms = timed(trace(O_a, D_a, channels=("t", "prim_id")))
    result["a_trace_rays_t_prim"] = {"rays": W * H, "ms": round(ms, 4), "rays_per_s": W * H / (ms * 1e-3)}
    ref_a = ctx.trace_rays(O_a, D_a, channels=("t", "prim_id"), stream=stream)
    torch.cuda.synchronize()
    result["a_equals_gbuffer"] = bool(torch.equal(ref_a["t"].view(torch.int32), gbuf["t"].reshape(-1).view(torch.int32))
                                      and torch.equal(ref_a["prim_id"], gbuf["prim_id"].reshape(-1)))
    result["a_ratio_to_gbuffer"] = round(result["a_trace_rays_t_prim"]["ms"] / result["a_gbuffer_t_prim"]["ms"], 3)

    # (b) incoherent rays
    arrs = hs.arrays()
    lo, hi = arrs["nodes"][0]["bbox_min"].astype(np.float64), arrs["nodes"][0]["bbox_max"].astype(np.float64)
    c, radius = 0.5 * (lo + hi), 0.5 * float(np.linalg.norm(hi - lo))
    rng = np.random.default_rng(2024)
    n = a.incoherent
    g = rng.normal(size=(n, 3))
    Ob = c + g / np.linalg.norm(g, axis=1, keepdims=True) * (2.0 * radius)
    Db = (lo + rng.random((n, 3)) * (hi - lo)) - Ob
    O_b = torch.from_numpy(Ob.astype(np.float32)).to(dev)
    D_b = torch.from_numpy(Db.astype(np.float32)).to(dev)
    ms = timed(trace(O_b, D_b, channels=("t", "prim_id")))
    ref_b = ctx.trace_rays(O_b, D_b, channels=("t", "prim_id"), stream=stream)
    torch.cuda.synchronize()
    result["b_incoherent_t_prim"] = {"rays": n, "ms": round(ms, 4), "rays_per_s": n / (ms * 1e-3), "hit_fraction": float((ref_b["prim_id"] >= 0).float().mean())}

    # (c) any-hit shadow rays of the frame's G-buffer hits
    full = ctx.trace_rays(O_a, D_a, channels=("position", "normal", "flags"), stream=stream)
    torch.cuda.synchronize()
    hitm = (full["flags"] & 1).bool()
    so = (full["position"] + full["normal"] * 1e-3)[hitm].contiguous()
    L = -torch.tensor(list(fr.sun_dir_model), dtype=torch.float64)
    L = (L / torch.linalg.norm(L)).float()
    sd = L.to(dev).expand(so.shape[0], 3).contiguous()
    ms = timed(trace(so, sd, any_hit=True))
    shadow = ctx.trace_rays(so, sd, any_hit=True, stream=stream)
    torch.cuda.synchronize()
    result["c_shadow_anyhit"] = {"rays": int(so.shape[0]), "ms": round(ms, 4), "rays_per_s": so.shape[0] / (ms * 1e-3),
                                 "blocked_fraction": float(shadow["flags"].float().mean())}

    ctx.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
