#!/usr/bin/env python3
"""Measurement (not a test): what the detector model costs (include/dsrt.h, SENSOR MODEL) at 1920x1080 and 3840x2160, psf_size 1, 9 and 33 (and no PSF), mono and
colour, on the linear frame of the test suite's station mesh (pose frame 98, rng_mode 1, 2 spp, the plain mean: only the post-pass is timed).  Device times are
HIP-event times on one stream around the operation, `--reps` launches after `--warmup`, configurations interleaved rep by rep; median, min and max.  Per size:
  sensor_<mono|colour>_psf<N>      dsrt_sensor_apply writing dn and rgb8 with every noise term on; the taps are the same from call to call, so the call is its one
                                   kernel launch (nothing is uploaded) and the event time is the kernel's plus the launch
  call_wall_ms                     host wall time of the same call and a stream synchronisation
  to_host_wall_ms                  dsrt_sensor_apply_to_host: the frame copied in, dn and rgb8 copied out
  atrous_iteration                 the yardstick: one a-trous iteration of the denoiser on the same frame (two iterations minus one, same run)
  ceilings_psf33                   for psf_size 33 the two ceilings of DESIGN.md section 4, from the micro-architecture tables and not from the kernel -- LDS reads (one
                                   ds_read_b32 per tap and plane for every FOUR pixels: the register window) and VALU issue (a multiply and an add per tap, plane and
                                   pixel, two pixels per packed instruction) -- and the measured time as a multiple of each
Prints one JSON line.

usage: tools/sensor_probe.py [--reps 20] [--warmup 3] [--wall-reps 5] [--frame 98] [--cus 256] [--clock-ghz 2.4]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((1920, 1080), (3840, 2160))
PSF_SIZES = (None, 1, 9, 33)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--wall-reps", type=int, default=5)
    ap.add_argument("--frame", type=int, default=98)
    ap.add_argument("--cus", type=int, default=256)
    ap.add_argument("--clock-ghz", type=float, default=2.4)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import dsrt_amd as d

    say = lambda what: print(f"[sensor_probe] {what}", file=sys.stderr, flush=True)   # noqa: E731
    assets = os.path.join(ROOT, "tests", "golden")
    hs = d.HostScene().add_obj(os.path.join(assets, "assets", "station_3k.obj"))
    hs.build_bvh()
    fr = d.pose_to_frame(d.read_pose_file(os.path.join(assets, "rendezvous_1s_dt0_01s.txt"))[a.frame])
    ctx = d.Context(0)
    ctx.upload(hs.view(d.frame_camera(fr, 40.0, SIZES[0][0], SIZES[0][1], 2, 50), tuple(fr.sun_dir_model)))       # (both rasters are 16:9: one camera)
    stream = torch.cuda.current_stream()
    raw = stream.cuda_stream
    noise = dict(prnu=0.01, dark_e=3.0, dsnu_e=2.0, read_e=12.0, noise=1, frame=3, seed=7)
    out = {"reps": a.reps, "sizes": {}}
    for W, H in SIZES:
        desc = d.make_desc(W, H, 2, 50, rng_mode=1)
        acc = d.Accumulator(ctx, desc, moments=True)
        acc.render(0, stream=raw)
        guides = acc.guides(stream=raw)
        lin = ctx.denoise_accumulated(desc, acc.sum, acc.sum_sq, guides, samples_done=2, params=d.denoise_defaults(iterations=0), want_rgb8=False, stream=raw)[2]
        torch.cuda.synchronize()
        say(f"{W}x{H}: frame rendered")
        params = {}
        for mono in (0, 1):
            for n in PSF_SIZES:
                psf = d.sensor_psf_gaussian(max(n / 6.0, 0.5), n) if n else None
                params[f"sensor_{'mono' if mono else 'colour'}_psf{n or 0}"] = d.sensor_defaults(psf=psf, mono=mono, **noise)
        outs = {k: (torch.empty((H, W) if p.mono else (H, W, 3), dtype=torch.uint16, device=lin.device), torch.empty((H, W, 3), dtype=torch.uint8, device=lin.device))
                for k, p in params.items()}

        def run(cfg):
            if cfg.startswith("atrous_"):
                ctx.denoise_accumulated(desc, acc.sum, acc.sum_sq, guides, samples_done=2, params=d.denoise_defaults(iterations=int(cfg[-1])), stream=raw)
            else:
                dn, rgb = outs[cfg]
                rc = d.lib.dsrt_sensor_apply(ctx._h, desc, lin.data_ptr(), params[cfg], dn.data_ptr(), None, rgb.data_ptr(), raw)
                assert rc == 0, d.lib.dsrt_last_error()

        cfgs = list(params) + ["atrous_1", "atrous_2"]
        ms, wall = {}, {}
        for rep in range(a.warmup + a.reps):
            k = rep % len(cfgs)
            for cfg in cfgs[k:] + cfgs[:k]:
                if not cfg.startswith("atrous_"):
                    run(cfg)                                                         # (the context keeps the last taps: this call uploads them, the timed one does not)
                    torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record(stream)
                run(cfg)
                e1.record(stream)
                e1.synchronize()
                if rep >= a.warmup:
                    ms.setdefault(cfg, []).append(e0.elapsed_time(e1))
                    wall.setdefault(cfg, []).append((time.perf_counter() - t0) * 1e3)
        med = {k: statistics.median(x) for k, x in ms.items()}
        row = {"median_ms": med, "min_ms": {k: min(x) for k, x in ms.items()}, "max_ms": {k: max(x) for k, x in ms.items()},
               "call_wall_ms": {k: statistics.median(x) for k, x in wall.items() if not k.startswith("atrous_")},
               "atrous_iteration_ms": med["atrous_2"] - med["atrous_1"]}
        say(f"{W}x{H}: launches timed")
        host = lin.cpu().numpy()
        to_host = {}
        for cfg in ("sensor_colour_psf0", "sensor_colour_psf33", "sensor_mono_psf33"):
            t = []
            for rep in range(1 + a.wall_reps):
                t0 = time.perf_counter()
                ctx.sensor_apply(desc, host, params[cfg], want_dn=True, want_rgb8=True)
                if rep:
                    t.append((time.perf_counter() - t0) * 1e3)
            to_host[cfg] = statistics.median(t)
        row["to_host_wall_ms"] = to_host
        # the two ceilings at psf_size 33, from the micro-architecture tables: a wave's ds_read_b32 takes 2 cycles of the CU's one LDS; a wave64 fp32 multiply or
        # add takes 2 cycles of one of the CU's four SIMD-32s (a packed one does two pixels in 4: the same rate per result, which is how 157 TF is the vector peak)
        ceil = {}
        for name, planes in (("colour", 3), ("mono", 1)):
            taps = 33 * 33
            waves = W * H / 64.0
            lds_reads = waves * planes * taps / 4.0                                  # wave-level ds_read_b32: one per tap and plane for FOUR pixels (the register window)
            valu = waves * planes * taps * 2                                         # wave-level multiplies and adds, counted unpacked: one of each per tap, plane and pixel
            lds_ms = lds_reads * 2 / (a.cus * a.clock_ghz * 1e9) * 1e3
            valu_ms = valu * 2 / (a.cus * 4 * a.clock_ghz * 1e9) * 1e3
            got = med[f"sensor_{name}_psf33"]
            ceil[name] = {"lds_wave_reads": lds_reads, "valu_wave_instructions": valu, "lds_ceiling_ms": lds_ms, "valu_ceiling_ms": valu_ms,
                          "measured_over_lds": got / lds_ms, "measured_over_valu": got / valu_ms}
        row["ceilings_psf33"] = ceil
        out["sizes"][f"{W}x{H}"] = row
    ctx.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
