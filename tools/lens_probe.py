#!/usr/bin/env python3
"""Measurement (not a test): what the lens model costs (include/dsrt.h, LENS MODEL) at 1920x1080 and 3840x2160, three channels, each filter, with every coefficient
zero and with a barrel (k1 -0.25, k2 0.05, p1 0.002, p2 -0.001, vignetting, cos^4), source and output of the same size, on a random frame (the pass needs no scene).
Device times are HIP-event times on one stream around the call, `--reps` launches after `--warmup`, configurations interleaved rep by rep; median, min and max.
Per size:
  lens_<nearest|linear|cubic>_<zero|barrel>   dsrt_lens_apply writing image, src_xy and status: one kernel launch
  lens_cubic_barrel_image_only                 the same writing the image alone
  sensor_colour_psf0                           the yardstick, in the same process: the detector's no-PSF colour call, also one streaming pass over the frame
  ceilings                                     from the micro-architecture tables and the kernel's ISA, not from a measurement: HBM -- the source read once and the
                                               outputs written once at --hbm-tbs -- and VALU issue -- the wave-level vector instructions of one pixel's path
                                               (counted in the gfx950 ISA of the three-channel instantiations: the twelve inverse steps are 37 each, unrolled by 3)
                                               at 2 cycles each on one of a CU's four SIMDs -- and the measured time as a multiple of each
Prints one JSON line.

usage: tools/lens_probe.py [--reps 20] [--warmup 3] [--cus 256] [--clock-ghz 2.4] [--hbm-tbs 6.3]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((1920, 1080), (3840, 2160))
FILTERS = ("nearest", "linear", "cubic")
VALU_PER_PIXEL = {"nearest": 555, "linear": 646, "cubic": 842}      # wave-level v_* instructions on the all-taps-inside path of dsrt_lens_kernel<3, filter>
BARREL = dict(k1=-0.25, k2=0.05, p1=0.002, p2=-0.001, v1=-0.3, v2=0.05, cos4=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cus", type=int, default=256)
    ap.add_argument("--clock-ghz", type=float, default=2.4)
    ap.add_argument("--hbm-tbs", type=float, default=6.3)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    import dsrt_amd as d

    say = lambda what: print(f"[lens_probe] {what}", file=sys.stderr, flush=True)   # noqa: E731
    ctx = d.Context(0)
    stream = torch.cuda.current_stream()
    raw = stream.cuda_stream
    out = {"reps": a.reps, "sizes": {}}
    for W, H in SIZES:
        desc = d.make_desc(W, H, 1)
        src = torch.rand((H, W, 3), dtype=torch.float32, device="cuda:0")
        f = 0.9 * W                                                                  # about 58 degrees across: the barrel's corners stay inside the fold-over
        frames = dict(src_width=W, src_height=H, src_fx=f, src_fy=f, src_cx=(W - 1) / 2, src_cy=(H - 1) / 2, fx=f, fy=f, cx=(W - 1) / 2, cy=(H - 1) / 2)
        params = {}
        for i, name in enumerate(FILTERS):
            params[f"lens_{name}_zero"] = d.lens_defaults(filter=i, **frames)
            params[f"lens_{name}_barrel"] = d.lens_defaults(filter=i, **frames, **BARREL)
        params["lens_cubic_barrel_image_only"] = d.lens_defaults(filter=2, **frames, **BARREL)
        image = torch.empty((H, W, 3), dtype=torch.float32, device=src.device)
        xy = torch.empty((H, W, 2), dtype=torch.float32, device=src.device)
        status = torch.empty((H, W), dtype=torch.uint8, device=src.device)
        full = d.capi.DsrtLensOut(image.data_ptr(), xy.data_ptr(), status.data_ptr())
        only = d.capi.DsrtLensOut(image.data_ptr(), None, None)
        sensor = d.sensor_defaults(prnu=0.01, dark_e=3.0, dsnu_e=2.0, read_e=12.0, noise=1, frame=3, seed=7)
        dn = torch.empty((H, W, 3), dtype=torch.uint16, device=src.device)
        rgb = torch.empty((H, W, 3), dtype=torch.uint8, device=src.device)

        def run(cfg):
            if cfg == "sensor_colour_psf0":
                rc = d.lib.dsrt_sensor_apply(ctx._h, desc, src.data_ptr(), sensor, dn.data_ptr(), None, rgb.data_ptr(), raw)
            else:
                rc = d.lib.dsrt_lens_apply(ctx._h, desc, src.data_ptr(), params[cfg], only if cfg.endswith("image_only") else full, raw)
            assert rc == 0, d.lib.dsrt_last_error()

        cfgs = list(params) + ["sensor_colour_psf0"]
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
        run("lens_cubic_barrel")
        torch.cuda.synchronize()
        row = {"median_ms": med, "min_ms": {k: min(x) for k, x in ms.items()}, "max_ms": {k: max(x) for k, x in ms.items()},
               "barrel_share_all_taps_inside": float((status == 7).float().mean()), "barrel_share_inverted": float(((status & 1) != 0).float().mean())}
        say(f"{W}x{H}: launches timed")
        px = W * H
        ceil = {}
        for name in FILTERS:
            bytes_moved = px * 12 + px * (12 + 8 + 1)                               # the source read once; image, src_xy and status written once
            hbm_ms = bytes_moved / (a.hbm_tbs * 1e12) * 1e3
            valu_ms = px / 64.0 * VALU_PER_PIXEL[name] * 2 / (a.cus * 4 * a.clock_ghz * 1e9) * 1e3
            got = med[f"lens_{name}_barrel"]
            ceil[name] = {"bytes": bytes_moved, "hbm_ceiling_ms": hbm_ms, "valu_wave_instructions_per_wave": VALU_PER_PIXEL[name], "valu_ceiling_ms": valu_ms,
                          "measured_over_hbm": got / hbm_ms, "measured_over_valu": got / valu_ms, "measured_over_sensor_psf0": got / med["sensor_colour_psf0"]}
        row["ceilings"] = ceil
        out["sizes"][f"{W}x{H}"] = row
    ctx.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
