#!/usr/bin/env python3
"""Timings of the tensor window decode entries next to what a caller does without them, both stream versions and both element types, through the ctypes view:

  python tools/windows_tensor_bench.py [--reps 7] [--warmup 2]

Workloads (photo-noise, synthesised on the device; three planes, the usual mean / std normalisation):
  crops   256 crops of 224 x 224 out of 64 streams of 1024^2 (four per stream, every second one block-aligned)
  whole   64 whole 512^2 images
Variants, alternating within a repetition so that box and clock are shared:
  (a) baseline  the batched RGBA window decode into an int32 N x h x w tensor, then the torch ops that make the N x 3 x h x w tensor of it: shift, mask and stack,
                to float32, multiply, add[, to float16]
  (b) fused     ONE call of limg_hip_*decode_stream_windows_tensor_device into the same shape
The two tensors are asserted bit-equal before anything is timed.  Each variant: HIP events on the launch stream around all of its work, min / median / max in ms
over the repetitions.  One JSON line per workload, version and type with baseline / fused by median, and the bytes per pixel each path moves by construction
(derived, not measured).  The first line says which build was measured."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def stats(v):
    v = sorted(v)
    return {"min": round(v[0], 4), "median": round(v[len(v) // 2], 4), "max": round(v[-1], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    assert args.reps >= 7 and args.warmup >= 2
    import torch
    import bench
    import limg_amd
    print(json.dumps(dict(tool="windows_tensor_bench", lib=os.path.basename(limg_amd.LIB_PATH), **bench.provenance())), flush=True)
    g = limg_amd.LimgHip(0)
    scale = [float(np.float32(1 / (255 * s))) for s in STD]
    bias = [float(np.float32(-m / s)) for m, s in zip(MEAN, STD)]
    d_scale = torch.tensor(scale, dtype=torch.float32, device="cuda").view(1, 3, 1, 1)
    d_bias = torch.tensor(bias, dtype=torch.float32, device="cuda").view(1, 3, 1, 1)

    def event_clock(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        return lambda: a.elapsed_time(b)

    for workload, n, streams, per_stream, side in (("crops", 1024, 64, 4, 224), ("whole", 512, 64, 1, 512)):
        imgs = [g.synth_device("photo_noise", n, n, seed=1 + i) for i in range(streams)]
        count = streams * per_stream
        rng = np.random.RandomState(7)
        wins = []
        for i in range(count):
            x, y = int(rng.randint(0, n - side + 1)), int(rng.randint(0, n - side + 1))
            if i % 2 == 0:
                x, y = x // 8 * 8, y // 8 * 8
            wins.append((x, y))
        for version in (1, 2):
            enc = [(g.encode_stream_device if version == 1 else g.blocked_encode_stream_device)(img, True) for img in imgs]
            torch.cuda.synchronize()
            rgba_entry = g.decode_stream_windows_device if version == 1 else g.blocked_decode_stream_windows_device
            rgba = torch.empty((count, side, side), dtype=torch.int32, device="cuda")
            rgba_jobs = [(enc[i % streams][0], enc[i % streams][1], n, n, *wins[i], side, side, rgba[i], side) for i in range(count)]
            crop_jobs = [(enc[i % streams][0], enc[i % streams][1], n, n, *wins[i]) for i in range(count)]
            for dtype in (torch.float32, torch.float16):
                fused_out = torch.empty((count, 3, side, side), dtype=dtype, device="cuda")
                result = {}

                def baseline():
                    rgba_entry(rgba_jobs)
                    planes = torch.stack([(rgba >> (8 * c)) & 0xFF for c in range(3)], dim=1).to(torch.float32)
                    out = planes * d_scale + d_bias  # two ops, each rounded on its own: the contract's expression
                    result["out"] = out if dtype == torch.float32 else out.to(torch.float16)

                def fused():
                    g.decode_crops_device(crop_jobs, side, side, dtype, scale, bias, planes=3, blocked=version == 2, out=fused_out)

                baseline()
                fused()
                torch.cuda.synchronize()
                g.check()
                bits = torch.int32 if dtype == torch.float32 else torch.int16
                assert torch.equal(result["out"].view(bits), fused_out.view(bits)), "the fused call and the baseline disagree"
                ms = {"baseline": [], "fused": []}
                for rep in range(args.warmup + args.reps):
                    for name, fn in (("baseline", baseline), ("fused", fused)):
                        t = event_clock(fn)
                        torch.cuda.synchronize()
                        if rep >= args.warmup:
                            ms[name].append(t())
                ms = {k: stats(v) for k, v in ms.items()}
                g.check()
                eb = 4 if dtype == torch.float32 else 2
                # derived, by construction: the baseline stores 4 B/px of RGBA, reads them back at least once and writes the three planes (the torch chain's own
                # intermediates come on top); the fused path writes the three planes only
                print(json.dumps({"workload": workload, "size": n, "version": version, "type": str(dtype).split(".")[-1], "windows": count, "streams": streams, "side": side,
                                  "reps": args.reps, "baseline_ms": ms["baseline"], "fused_ms": ms["fused"],
                                  "baseline_over_fused": round(ms["baseline"]["median"] / ms["fused"]["median"], 3),
                                  "fused_not_above_baseline": ms["fused"]["median"] <= ms["baseline"]["median"],
                                  "derived_bytes_per_pixel": {"baseline_at_least": 4 + 4 + 3 * eb, "fused": 3 * eb}}), flush=True)
                del fused_out, result
            del enc, rgba, rgba_jobs, crop_jobs
            torch.cuda.empty_cache()
        del imgs
        torch.cuda.empty_cache()
    g.close()


if __name__ == "__main__":
    main()
