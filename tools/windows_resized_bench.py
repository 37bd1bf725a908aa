#!/usr/bin/env python3
"""Timings of the resized tensor window decode next to the route a caller had without it, both stream versions, float16, three planes, through the ctypes view:

  python tools/windows_resized_bench.py [--reps 7] [--warmup 2] [--out profiles/window_decode_resized.md]

Workloads (photo-noise, synthesised on the device; the usual mean / std normalisation):
  loader      256 seeded RandomResizedCrop rectangles (area 0.08 .. 1 of the image, aspect 3/4 .. 4/3, every second one mirrored) out of four 2048^2 streams to 224^2.
              The rectangles are rounded to multiples of 8 pixels so that the yardstick's footprint is the rectangle itself at every level
  thumbnail   the 1000 x 1000 thumbnail of one 8192^2 stream
Variants, alternating within a repetition so that box and clock are shared:
  (a) yardstick  per job limg_hip_*decode_stream_windows_scaled_tensor_device at the level the resized entry picks, on the job's footprint, then
                 torch.nn.functional.interpolate(bilinear, align_corners=False) per sample to the output size, and the flip
  (b) resized    ONE decode_crops_resized_device call
The two results are compared before anything is timed.  Bound: the contract's 1.52 byte steps (times the largest scale) against exact bilinear, plus the yardstick's
own rounding: its float16 input (half an ulp), its float16 result (half an ulp) and the resized entry's own float16 result (half an ulp) at magnitudes below 4, where
an ulp is 2^-9 -- 2^-8 in all.  Each variant: HIP events on the launch stream around all of its work, min / median / max in ms over the repetitions.  One JSON line per
workload and version; --out also writes them as the profile's table, with the bytes of intermediate the yardstick allocates and the tile capacity."""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
TILE_PIXELS = 4096  # kResizeTilePixels (limg_amd/csrc/limg_hip_internal.h)


def stats(v):
    v = sorted(v)
    return {"min": round(v[0], 4), "median": round(v[len(v) // 2], 4), "max": round(v[-1], 4)}


def auto_level(sw, sh, ow, oh):
    L = 0
    while L < 3 and (sw >> (L + 1)) >= ow and (sh >> (L + 1)) >= oh:
        L += 1
    return L


def random_resized_crops(n, size, seed):
    """torchvision's RandomResizedCrop sampling (area 0.08 .. 1, log-uniform aspect 3/4 .. 4/3), seeded, rounded to multiples of 8"""
    rng = np.random.RandomState(seed)
    out = []
    while len(out) < n:
        area = size * size * rng.uniform(0.08, 1.0)
        aspect = math.exp(rng.uniform(math.log(3 / 4), math.log(4 / 3)))
        w, h = int(round(math.sqrt(area * aspect))) // 8 * 8, int(round(math.sqrt(area / aspect))) // 8 * 8
        if 8 <= w <= size and 8 <= h <= size:
            out.append((int(rng.randint(0, (size - w) // 8 + 1)) * 8, int(rng.randint(0, (size - h) // 8 + 1)) * 8, w, h, bool(len(out) & 1)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.reps >= 7 and args.warmup >= 2
    import torch
    import bench
    import limg_amd
    head = dict(tool="windows_resized_bench", lib=os.path.basename(limg_amd.LIB_PATH), tile_pixels=TILE_PIXELS, **bench.provenance())
    print(json.dumps(head), flush=True)
    g = limg_amd.LimgHip(0)
    scale = [float(np.float32(1 / (255 * s))) for s in STD]
    bias = [float(np.float32(-m / s)) for m, s in zip(MEAN, STD)]
    fmt = limg_amd.tensor_format(torch.float16, 3, scale, bias)
    tolerance = 1.52 * max(scale) + 2.0 ** -8

    def event_clock(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        return lambda: a.elapsed_time(b)

    lines = []
    for version in (1, 2):
        blocked = version == 2
        scaled_entry = g.blocked_decode_stream_windows_scaled_tensor_device if blocked else g.decode_stream_windows_scaled_tensor_device
        for workload, size, n_streams, side, rects in (("loader", 2048, 4, 224, random_resized_crops(256, 2048, 7)), ("thumbnail", 8192, 1, 1000, [(0, 0, 8192, 8192, False)])):
            enc = []
            for i in range(n_streams):
                img = g.synth_device("photo_noise", size, size, seed=1 + i)
                enc.append((g.blocked_encode_stream_device if blocked else g.encode_stream_device)(img, True))
                torch.cuda.synchronize()
                del img
            torch.cuda.empty_cache()
            out_a = torch.empty((len(rects), 3, side, side), dtype=torch.float16, device="cuda")
            out_b = torch.empty_like(out_a)
            levels = [auto_level(w, h, side, side) for _, _, w, h, _ in rects]
            inter = [torch.empty((3, h >> L, w >> L), dtype=torch.float16, device="cuda") for (_, _, w, h, _), L in zip(rects, levels)]
            scaled_jobs = [[(enc[i % n_streams][0], enc[i % n_streams][1], size, size, L, x >> L, y >> L, w >> L, h >> L, inter[i], None, None)]
                           for i, ((x, y, w, h, _), L) in enumerate(zip(rects, levels))]
            resized_jobs = [(enc[i % n_streams][0], enc[i % n_streams][1], size, size, x, y, w, h, flip) for i, (x, y, w, h, flip) in enumerate(rects)]

            def yardstick():
                for i, (_, _, _, _, flip) in enumerate(rects):
                    scaled_entry(scaled_jobs[i], fmt)
                    s = torch.nn.functional.interpolate(inter[i][None], size=(side, side), mode="bilinear", align_corners=False)[0]
                    out_a[i] = torch.flip(s, dims=(2,)) if flip else s

            def resized():
                g.decode_crops_resized_device(resized_jobs, side, side, torch.float16, scale, bias, planes=3, blocked=blocked, out=out_b)

            yardstick()
            resized()
            torch.cuda.synchronize()
            g.check()
            worst = float((out_a.float() - out_b.float()).abs().max())
            assert worst <= tolerance, ("the resized call and the yardstick disagree", worst, tolerance)
            ms = {"yardstick": [], "resized": []}
            for rep in range(args.warmup + args.reps):
                for name, fn in (("yardstick", yardstick), ("resized", resized)):
                    t = event_clock(fn)
                    torch.cuda.synchronize()
                    if rep >= args.warmup:
                        ms[name].append(t())
            ms = {n: stats(v) for n, v in ms.items()}
            g.check()
            line = {"workload": workload, "size": size, "version": version, "jobs": len(rects), "streams": n_streams, "side": side, "levels": sorted(set(levels)), "reps": args.reps,
                    "worst_difference": round(worst, 5), "tolerance": round(tolerance, 5), "yardstick_intermediate_bytes": int(sum(t.numel() * 2 for t in inter)),
                    "yardstick_ms": ms["yardstick"], "resized_ms": ms["resized"], "yardstick_over_resized": round(ms["yardstick"]["median"] / ms["resized"]["median"], 3)}
            print(json.dumps(line), flush=True)
            lines.append(line)
            del enc, inter, out_a, out_b, scaled_jobs, resized_jobs
            torch.cuda.empty_cache()
    g.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("# Resized window decode: one fused call against scaled decode + interpolate per sample\n\n")
            f.write("Written by `tools/windows_resized_bench.py` (HIP events, %d warm-up + %d repetitions, the variants alternating in one process; times in ms as min / median / max).\n" % (args.warmup, args.reps))
            f.write("Yardstick: per job the scaled tensor entry at the job's level on its footprint, `torch.nn.functional.interpolate(bilinear)` to the output size, the flip.\n")
            f.write("Resized: ONE `decode_crops_resized_device` call.  float16, 3 planes.  LDS tile capacity: %d level pixels (16 KiB).\n\n" % TILE_PIXELS)
            f.write("`%s`\n\n" % json.dumps(head))
            f.write("| workload | version | jobs | levels | yardstick ms | resized ms | yardstick / resized | yardstick intermediate bytes | worst difference (bound) |\n|---|---|---|---|---|---|---|---|---|\n")
            for ln in lines:
                fm = lambda s: "%.3f / %.3f / %.3f" % (s["min"], s["median"], s["max"])
                f.write("| %s %d^2 -> %d^2 | %d | %d | %s | %s | %s | %.3f | %d | %.5f (%.5f) |\n" % (ln["workload"], ln["size"], ln["side"], ln["version"], ln["jobs"], ln["levels"], fm(ln["yardstick_ms"]),
                                                                                              fm(ln["resized_ms"]), ln["yardstick_over_resized"], ln["yardstick_intermediate_bytes"],
                                                                                              ln["worst_difference"], ln["tolerance"]))


if __name__ == "__main__":
    main()
