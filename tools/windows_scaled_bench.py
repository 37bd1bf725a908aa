#!/usr/bin/env python3
"""Timings of the reduced-scale tensor window decode next to the route a caller had without it, both stream versions, float32, through the ctypes view:

  python tools/windows_scaled_bench.py [--reps 7] [--warmup 2] [--streams 4]

Workloads (photo-noise, synthesised on the device; three planes, the usual mean / std normalisation):
  crops       64 crops whose source footprint is 1792 x 1792 out of `--streams` streams of 8192^2, at levels 0 .. 3: 1792^2, 896^2, 448^2 and 224^2 output
  thumbnail   the whole level-3 image (1024^2) of one 8192^2 stream
Variants, alternating within a repetition so that box and clock are shared:
  (a) parent    limg_hip_*decode_stream_windows_tensor_device at full scale on the same footprint, then torch.nn.functional.avg_pool2d(k) (nothing at level 0)
  (b) scaled    ONE call of limg_hip_*decode_stream_windows_scaled_tensor_device
The two results are compared before anything is timed: bit-equal at level 0; elsewhere the parent route averages in float where the scaled entry rounds the byte mean
half up, so they may differ by up to half a byte step times the scale (plus float rounding) and no more.  Each variant: HIP events on the launch stream around all of
its work, min / median / max in ms over the repetitions.  One JSON line per workload, version and level; `scaled_not_above_level0` states whether the level's call is
no slower (by median) than the level-0 call on the same footprint.  The first line says which build was measured."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SIZE, FOOT, CROPS = 8192, 1792, 64


def stats(v):
    v = sorted(v)
    return {"min": round(v[0], 4), "median": round(v[len(v) // 2], 4), "max": round(v[-1], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--streams", type=int, default=4)
    args = ap.parse_args()
    assert args.reps >= 7 and args.warmup >= 2 and 1 <= args.streams <= CROPS
    import torch
    import bench
    import limg_amd
    print(json.dumps(dict(tool="windows_scaled_bench", lib=os.path.basename(limg_amd.LIB_PATH), **bench.provenance())), flush=True)
    g = limg_amd.LimgHip(0)
    scale = [float(np.float32(1 / (255 * s))) for s in STD]
    bias = [float(np.float32(-m / s)) for m, s in zip(MEAN, STD)]
    fmt = limg_amd.tensor_format(torch.float32, 3, scale, bias)
    tolerance = 0.5 * max(scale) * 1.001 + 1e-5

    def event_clock(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        return lambda: a.elapsed_time(b)

    rng = np.random.RandomState(7)
    origins = []  # of the footprints, multiples of 8 in source pixels: a valid origin at every level
    for i in range(CROPS):
        origins.append((int(rng.randint(0, (SIZE - FOOT) // 8 + 1)) * 8, int(rng.randint(0, (SIZE - FOOT) // 8 + 1)) * 8))

    for version in (1, 2):
        blocked = version == 2
        enc = []
        for i in range(args.streams):
            img = g.synth_device("photo_noise", SIZE, SIZE, seed=1 + i)
            enc.append((g.blocked_encode_stream_device if blocked else g.encode_stream_device)(img, True))
            torch.cuda.synchronize()
            del img
        torch.cuda.empty_cache()
        full_entry = g.blocked_decode_stream_windows_tensor_device if blocked else g.decode_stream_windows_tensor_device
        for workload, jobs_of in (("crops", lambda L: [(enc[i % len(enc)], origins[i][0] >> L, origins[i][1] >> L, FOOT >> L) for i in range(CROPS)]),
                                  ("thumbnail", lambda L: [(enc[0], 0, 0, SIZE >> L)])):
            level0_median = None
            for L in ((0, 1, 2, 3) if workload == "crops" else (3,)):
                k = 1 << L
                jobs = jobs_of(L)
                side, src = jobs[0][3], jobs[0][3] << L
                full = torch.empty((len(jobs), 3, src, src), dtype=torch.float32, device="cuda")
                out = torch.empty((len(jobs), 3, side, side), dtype=torch.float32, device="cuda")
                full_jobs = [(st, nb, SIZE, SIZE, x << L, y << L, src, src, full[i], src, src * src) for i, ((st, nb), x, y, _) in enumerate(jobs)]
                crop_jobs = [(st, nb, SIZE, SIZE, L, x, y) for (st, nb), x, y, _ in jobs]
                result = {}

                def parent():
                    full_entry(full_jobs, fmt)
                    result["out"] = full if L == 0 else torch.nn.functional.avg_pool2d(full, k)

                def scaled():
                    g.decode_crops_scaled_device(crop_jobs, side, side, torch.float32, scale, bias, planes=3, blocked=blocked, out=out)

                parent()
                scaled()
                torch.cuda.synchronize()
                g.check()
                if L == 0:
                    assert torch.equal(result["out"].view(torch.int32), out.view(torch.int32)), "level 0 and the full-scale entry disagree"
                else:
                    worst = float((result["out"] - out).abs().max())
                    assert worst <= tolerance, ("the scaled call and the parent route disagree", worst, tolerance)
                ms = {"parent": [], "scaled": []}
                for rep in range(args.warmup + args.reps):
                    for name, fn in (("parent", parent), ("scaled", scaled)):
                        t = event_clock(fn)
                        torch.cuda.synchronize()
                        if rep >= args.warmup:
                            ms[name].append(t())
                ms = {n: stats(v) for n, v in ms.items()}
                g.check()
                if L == 0:
                    level0_median = ms["scaled"]["median"]
                line = {"workload": workload, "size": SIZE, "version": version, "level": L, "windows": len(jobs), "streams": len(enc) if workload == "crops" else 1,
                        "footprint": src, "side": side, "reps": args.reps, "parent_ms": ms["parent"], "scaled_ms": ms["scaled"],
                        "parent_over_scaled": round(ms["parent"]["median"] / ms["scaled"]["median"], 3)}
                if level0_median is not None and L > 0:
                    line["scaled_not_above_level0"] = ms["scaled"]["median"] <= level0_median
                print(json.dumps(line), flush=True)
                del full, out, result, full_jobs
                torch.cuda.empty_cache()
        del enc
        torch.cuda.empty_cache()
    g.close()


if __name__ == "__main__":
    main()
