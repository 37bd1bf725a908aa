#!/usr/bin/env python3
"""Timings of the batched stream encode next to the loop of single-image stream encodes it replaces, through the ctypes view:

  python tools/stream_batch_bench.py [--reps 7] [--warmup 2] [--lists NAME,NAME]

Lists (synthesised on the device, RGBA, default arguments): g4096 = 64 x 4096^2 random-gradient, p4096 = 64 x 4096^2 photo-noise, p1024 = 16 x 1024^2 photo-noise,
p512 = 256 x 512^2 photo-noise.
Variants, alternating within a repetition so that box and clock are shared:
  (a) loop     limg_hip_encode_stream_device once per image: four launches per image, ramp-up and drain per image.  This is code the batched entry does not touch --
               the single-image kernels' instructions are what they were before it existed -- so it is the yardstick.
  (b) batched  ONE call of limg_hip_encode_stream_batch_device
Neither asks for the sizes (no host wait inside the timed region).  Before anything is timed every stream of (b) is compared with (a)'s, byte for byte, up to its
header's totalBytes.  Each variant: HIP events on the launch stream around all of its calls, min / median / max in ms over the repetitions; Gpixel/s from the median.
One JSON line per list; the first line says which build was measured."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LISTS = {"g4096": ("random_gradient", 4096, 64), "p4096": ("photo_noise", 4096, 64), "p1024": ("photo_noise", 1024, 16), "p512": ("photo_noise", 512, 256)}


def stats(v):
    v = sorted(v)
    return {"min": round(v[0], 4), "median": round(v[len(v) // 2], 4), "max": round(v[-1], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--lists", default=",".join(LISTS))
    args = ap.parse_args()
    assert args.reps >= 7 and args.warmup >= 2
    import torch
    import bench
    import limg_amd
    print(json.dumps(dict(tool="stream_batch_bench", lib=os.path.basename(limg_amd.LIB_PATH), **bench.provenance())), flush=True)
    g = limg_amd.LimgHip(0)
    for name in args.lists.split(","):
        kind, n, count = LISTS[name]
        imgs = [g.synth_device(kind, n, n, seed=1 + i) for i in range(count)]
        bound = g.stream_bound(n, n)
        outs = [[torch.empty(bound, dtype=torch.uint8, device="cuda") for _ in range(count)] for _ in (0, 1)]

        def loop():
            for img, out in zip(imgs, outs[0]):
                g.encode_stream_device(img, True, out=out, want_size=False)

        def batched():
            g.encode_stream_batch_device(imgs, True, outs=outs[1], want_sizes=False)

        loop()
        batched()
        torch.cuda.synchronize()
        g.check()
        total = 0
        for a, b in zip(*outs):
            nbytes = int(a[:64].cpu().numpy().view(limg_amd.STREAM_HEADER_DTYPE)[0]["totalBytes"])
            assert torch.equal(a[:nbytes], b[:nbytes]), "the batched call and the loop disagree"
            total += nbytes
        ms = {"loop": [], "batched": []}
        for rep in range(args.warmup + args.reps):
            for key, fn in (("loop", loop), ("batched", batched)):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                if rep >= args.warmup:
                    ms[key].append(a.elapsed_time(b))
        g.check()
        ms = {k: stats(v) for k, v in ms.items()}
        gpx = {k: round(count * n * n / (v["median"] * 1e6), 2) for k, v in ms.items()}
        print(json.dumps({"list": name, "kind": kind, "size": n, "images": count, "reps": args.reps, "stream_bytes": total, "loop_ms": ms["loop"], "batched_ms": ms["batched"],
                          "gpixel_per_s": gpx, "loop_over_batched": round(ms["loop"]["median"] / ms["batched"]["median"], 3)}), flush=True)
        del imgs, outs
        torch.cuda.empty_cache()
    g.close()


if __name__ == "__main__":
    main()
