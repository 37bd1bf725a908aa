#!/usr/bin/env python3
"""Timings of the batched window decode entries next to the loop of single-window calls they replace, both stream versions, through the ctypes view:

  python tools/windows_decode_bench.py [--reps 7] [--warmup 2] [--no-host]

Workloads (photo-noise, synthesised on the device):
  tiles   64 seeded 256 x 256 windows of ONE 8192^2 stream, every second one block-aligned, the others anywhere
  crops   one such window from each of 16 different 2048^2 streams
Variants, alternating within a repetition so that box and clock are shared:
  (a) loop     the single-window entry once per window (limg_hip_*decode_stream_window_device): the yardstick
  (b) batched  ONE call of limg_hip_*decode_stream_windows_device
Each variant: HIP events on the launch stream around all of its calls, min / median / max in ms over the repetitions.  One JSON line per workload and version, with
(a) / (b) by median and, for version 2, the algorithmic bytes of the rectangle table scan: 64 B per rectangle, per window in (a), per distinct stream in (b).
The host forms are measured once, on the tiles workload in version 1, by the wall clock (they block): 64 calls of limg_hip_decode_stream_window, each uploading the whole
stream, against one limg_hip_decode_stream_windows.  The first line says which build was measured."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(v):
    v = sorted(v)
    return {"min": round(v[0], 4), "median": round(v[len(v) // 2], 4), "max": round(v[-1], 4)}


def seeded_windows(n, count, seed):
    rng = np.random.RandomState(seed)
    out = []
    for i in range(count):
        x, y = int(rng.randint(0, n - 256 + 1)), int(rng.randint(0, n - 256 + 1))
        if i % 2 == 0:
            x, y = x // 8 * 8, y // 8 * 8
        out.append((x, y, 256, 256))
    return out


def timed(variants, reps, warmup, sync, clock):
    ms = {k: [] for k in variants}
    for rep in range(warmup + reps):
        for name, fn in variants.items():
            t = clock(fn)
            sync()
            if rep >= warmup:
                ms[name].append(t())
    return {k: stats(v) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-host", action="store_true", help="skip the host forms (they move the 8192^2 stream over PCIe 64 times per repetition)")
    args = ap.parse_args()
    assert args.reps >= 7 and args.warmup >= 2
    import torch
    import bench
    import limg_amd
    print(json.dumps(dict(tool="windows_decode_bench", lib=os.path.basename(limg_amd.LIB_PATH), **bench.provenance())), flush=True)
    g = limg_amd.LimgHip(0)

    def event_clock(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        return lambda: a.elapsed_time(b)

    def wall_clock(fn):
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        return lambda: (t1 - t0) * 1e3

    def encode(img, version):
        if version == 1:
            st, nbytes = g.encode_stream_device(img, True)
            return st, nbytes, None
        st, nbytes = g.blocked_encode_stream_device(img, True)
        return st, nbytes, len(g.blocked_regions())

    host_stream = None
    for workload, n, streams in (("tiles", 8192, 1), ("crops", 2048, 16)):
        imgs = [g.synth_device("photo_noise", n, n, seed=1 + i) for i in range(streams)]
        count = 64 if streams == 1 else streams
        wins = seeded_windows(n, count, seed=7)
        outs = torch.empty((2, count, 256, 256), dtype=torch.int32, device="cuda")
        for version in (1, 2):
            enc = [encode(img, version) for img in imgs]
            torch.cuda.synchronize()
            single = g.decode_stream_window_device if version == 1 else g.blocked_decode_stream_window_device
            batched = g.decode_stream_windows_device if version == 1 else g.blocked_decode_stream_windows_device
            jobs = [[(enc[i % streams][0], enc[i % streams][1], n, n, *wins[i], outs[v, i], 256) for i in range(count)] for v in (0, 1)]

            def loop():
                for j in jobs[0]:
                    single(*j[:8], out=j[8], out_stride=j[9])

            ms = timed({"loop": loop, "batched": lambda: batched(jobs[1])}, args.reps, args.warmup, torch.cuda.synchronize, event_clock)
            g.check()
            assert torch.equal(outs[0], outs[1]), "the batched call and the loop disagree"
            line = {"workload": workload, "size": n, "version": version, "windows": count, "streams": streams, "reps": args.reps, "loop_ms": ms["loop"], "batched_ms": ms["batched"],
                    "loop_over_batched": round(ms["loop"]["median"] / ms["batched"]["median"], 3)}
            if version == 2:
                rects = [e[2] for e in enc]
                line["table_scan_bytes"] = {"loop": 64 * sum(rects[i % streams] for i in range(count)), "batched": 64 * sum(rects)}
            print(json.dumps(line), flush=True)
            if workload == "tiles" and version == 1 and not args.no_host:
                host_stream = enc[0][0][:enc[0][1]].cpu().numpy()
            del enc, jobs
            torch.cuda.empty_cache()
        if host_stream is not None:
            bufs = np.zeros((2, count, 256, 256), dtype=np.uint32)

            def host_loop():
                for i, (x, y, w, h) in enumerate(wins):
                    g.decode_stream_window(host_stream, x, y, w, h, out=bufs[0, i])

            ms = timed({"loop": host_loop, "batched": lambda: g.decode_stream_windows(host_stream, wins, outs=list(bufs[1]))}, args.reps, args.warmup, lambda: None, wall_clock)
            assert np.array_equal(bufs[0], bufs[1])
            print(json.dumps({"workload": "tiles, host form", "size": n, "version": 1, "windows": count, "stream_bytes": int(host_stream.size), "reps": args.reps, "clock": "wall",
                              "loop_ms": ms["loop"], "batched_ms": ms["batched"], "loop_over_batched": round(ms["loop"]["median"] / ms["batched"]["median"], 3)}), flush=True)
            host_stream = None
        del imgs, outs
        torch.cuda.empty_cache()
    g.close()


if __name__ == "__main__":
    main()
