#!/usr/bin/env python3
"""Measurement (not a test): what a pose update of a movable rigid body costs (include/dsrt.h, MOVABLE RIGID BODIES) -- the bench's 1,000,000-triangle stand-in
station as body 0 and a second, smaller copy of the station of `--body-tris` triangles (default 10^4, 10^5, 10^6) as body 1, pose frame 98.  Per body size:
  update_ms           dsrt_scene_set_body_poses, the `ms` it returns (HIP events around its launches) and the split: transform, refit (all depths), chain;
                      `--reps` calls after `--warmup`, a different pose each, medians with min and max; update_wall_ms is a host clock around the same (synchronous) call
  transform_GBps      the bytes the transform kernel reads and writes (400 per pair record: 160 rest, 32 ids, 80 + 96 + 32 written) over its median time, beside
                      copy_GBps, dsrt_microbench_copy on the same board in the same run
  rebuild_ms          the only route without resident bodies, same session, same scene: dsrt_host_scene_set_body_poses, dsrt_host_scene_build_bvh_gpu, dsrt_scene_upload
                      (host wall times, `--rebuild-reps` of them, median; the three parts separately)
  frame_ms            kernel_ms of a 1920x1080 x 64 spp rng_mode 1 frame on the bodies tree and on the median tree over the same posed triangles, alternating,
                      `--frame-reps` each, medians: what the fixed topology and the chain cost the traversal
Prints one JSON line per body size.

usage: tools/bodies_probe.py [--body-tris 10000 100000 1000000] [--reps 20] [--warmup 3] [--rebuild-reps 3] [--frame-reps 3] [--tris 1000000] [--frame 98] [--spp 64]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BYTES_PER_ENTRY = 160 + 32 + 80 + 96 + 32


def station_obj(meshgen, tris):
    obj = f"/tmp/dsrt_bench_station_v{meshgen.VERSION}_{tris}.obj"
    if not os.path.exists(obj):
        tmp = obj + f".{os.getpid()}.tmp"
        meshgen.write_obj(meshgen.build_station(tris), tmp, mtl_name=os.path.basename(obj)[:-4] + ".mtl")
        os.replace(tmp, obj)
    return obj


def pose(k, where):
    """A rotation by k-dependent angle about a skew axis, and a translation to `where`."""
    a = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    t = 0.1 + 0.37 * k
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)
    return np.concatenate([R, np.asarray(where, np.float64).reshape(3, 1)], axis=1).astype(np.float32).reshape(1, 12)


def med(x):
    return {"median": statistics.median(x), "min": min(x), "max": max(x)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--body-tris", type=int, nargs="+", default=[10000, 100000, 1000000])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rebuild-reps", type=int, default=3)
    ap.add_argument("--frame-reps", type=int, default=3)
    ap.add_argument("--tris", type=int, default=1000000)
    ap.add_argument("--frame", type=int, default=98)
    ap.add_argument("--spp", type=int, default=64)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import dsrt_amd as d
    from dsrt_amd import meshgen
    say = lambda what: print(f"[bodies_probe] {what}", file=sys.stderr, flush=True)   # noqa: E731
    W, H, depth = 1920, 1080, 50
    fr = d.pose_to_frame(d.read_pose_file(os.path.join(ROOT, "tests", "golden", "rendezvous_1s_dt0_01s.txt"))[a.frame])
    cam = d.frame_camera(fr, 40.0, W, H, a.spp, depth)
    sun = tuple(fr.sun_dir_model)
    where = 0.4 * np.array(fr.cam_in_model[:], np.float64)              # the visitor: between the camera and the station, in the picture
    station = station_obj(meshgen, a.tris)
    copy = d.microbench_copy()
    say(f"copy bandwidth {copy['GBps']:.0f} GB/s")
    desc = d.make_desc(W, H, a.spp, depth, rng_mode=1)
    for n in a.body_tris:
        body = station_obj(meshgen, n)
        hs = d.HostScene().add_obj(station)
        hs.begin_body()
        hs.add_obj(body, 0.25)
        t0 = time.perf_counter()
        hs.build_bvh_bodies()
        build_s = time.perf_counter() - t0
        first, count = hs.body_range(1)
        ctx = d.Context(0)
        ctx.upload_bodies(hs, hs.view(cam, sun))
        say(f"{n}: {count} body triangles on {first} static ones uploaded (bodies tree built in {build_s:.2f} s)")
        ms = {"total": [], "transform": [], "refit": [], "chain": [], "wall": []}
        for k in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            got = ctx.set_body_poses(1, pose(k, where), want_ms=True)
            wall = (time.perf_counter() - t0) * 1e3
            if k >= a.warmup:
                for key, v in zip(("total", "transform", "refit", "chain"), got):
                    ms[key].append(v)
                ms["wall"].append(wall)
        entries = (count + 1) // 2                                       # (a lower bound: every leaf of odd size ends in a half-empty record)
        row = {"body_tris": count, "static_tris": first, "stack_need": hs.stack_need, "reps": a.reps,
               "update_ms": {k: med(v) for k, v in ms.items() if k != "wall"}, "update_wall_ms": med(ms["wall"]),
               "transform_GBps_at_least": entries * BYTES_PER_ENTRY / (statistics.median(ms["transform"]) * 1e6), "copy_GBps": copy["GBps"]}
        # the frame on the bodies tree, posed as the last update left it, against the median tree over the same triangles
        last = pose(a.warmup + a.reps - 1, where)
        hs.set_body_poses(1, last)
        hs.build_bvh("median")
        flat = d.Context(0)
        flat.upload(hs.view(cam, sun))
        frame = {"bodies_tree": [], "median_tree": []}
        same = None
        for k in range(1 + a.frame_reps):
            for name, c in (("bodies_tree", ctx), ("median_tree", flat)):
                rgb, _, st = c.render_to_host(desc)
                if k:
                    frame[name].append(st.kernel_ms)
                elif name == "bodies_tree":
                    same = rgb
                else:
                    row["frames_differ_pixels"] = int((rgb != same).any(axis=2).sum())   # another tree: ties and grazing hits may resolve differently
        row["frame_ms"] = {k: med(v) for k, v in frame.items()}
        row["frame_cost_ratio"] = statistics.median(frame["bodies_tree"]) / statistics.median(frame["median_tree"])
        # the route without resident bodies: pose on the host, rebuild on the GPU, pack and upload everything
        t_host, t_build, t_upload = [], [], []
        for k in range(a.rebuild_reps):
            hs.build_bvh_bodies()                                        # posing needs the bodies tree back (not timed; the last pose becomes the rest pose: the cost is the same)
            t0 = time.perf_counter()
            hs.set_body_poses(1, last)
            t1 = time.perf_counter()
            hs.build_bvh("lbvh")
            t2 = time.perf_counter()
            flat.upload(hs.view(cam, sun))
            t3 = time.perf_counter()
            t_host.append((t1 - t0) * 1e3)
            t_build.append((t2 - t1) * 1e3)
            t_upload.append((t3 - t2) * 1e3)
        row["rebuild_ms"] = {"host_pose": med(t_host), "build_bvh_gpu": med(t_build), "upload": med(t_upload),
                             "total_median": statistics.median([x + y + z for x, y, z in zip(t_host, t_build, t_upload)])}
        print(json.dumps(row), flush=True)
        ctx.close()
        flat.close()
        hs.close()


if __name__ == "__main__":
    main()
