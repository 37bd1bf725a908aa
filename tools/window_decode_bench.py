#!/usr/bin/env python3
"""Timings of the window decode entries next to the full decoders, both stream versions, through the ctypes view:

  python tools/window_decode_bench.py [--reps 7] [--warmup 2]

For 8192^2 photo-noise and 4096^2 gradient, in version 1 and version 2 of the stream, it prints one JSON line with four variants:
  (a) full       the full decode entry (limg_hip_decode_stream_device / limg_hip_blocked_decode_stream_device; version 2's runs the kernels of (b))
  (b) whole      the window entry with the window = the whole image
  (c) aligned    a 1024^2 block-aligned window at (1024, 2048)
  (d) unaligned  a 1000 x 1000 window at (123, 457) into an odd stride, pOut 4 bytes off a 16-byte boundary
Each variant: HIP events on the launch stream around one call, min / median / max in ms over the repetitions; the variants alternate within a repetition, so box and
clock are shared.  With each: the algorithmic bytes -- table entries read (version 1: 56 B per block of the window's block range; version 2: the whole table, 64 B
per rectangle), the payload of the window's blocks (from the stream's own table), 4 B per pixel stored, and for version 2 the window's block map (4 B per block: set,
claimed, read = 12 B) -- and the share of the HBM peak (8 TB/s, MI355X) those bytes over the median time come to.  The first line says which build was measured."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12


def stats(v):
    v = sorted(v)
    return {"min": round(v[0], 4), "median": round(v[len(v) // 2], 4), "max": round(v[-1], 4)}


def field_bytes_per_block(shift):
    """payload bytes of one whole 8x8 block from a table's shift words: 8 rows x b bytes per field (b = 8 - shift; 8 where escaped; none at shift 8 without escape)"""
    total = np.zeros(shift.shape, dtype=np.int64)
    for k in range(3):
        s = ((shift >> (8 * k)) & 0xFF).astype(np.int64)
        esc = ((shift >> (24 + k)) & 1).astype(np.int64)
        total += np.where(s >= 8, 8 * esc, 8 - s) * 8
    return total


def block_range(win):
    x, y, w, h = win
    return x // 8, y // 8, (x + w - 1) // 8, (y + h - 1) // 8


def bytes_v1(table, blocks_x, win):
    bx0, by0, bx1, by1 = block_range(win)
    per_block = field_bytes_per_block(table["shift"]).reshape(-1, blocks_x)[by0:by1 + 1, bx0:bx1 + 1]
    blocks = per_block.size
    return {"table": 56 * blocks, "payload": int(per_block.sum()), "stored": 4 * win[2] * win[3]}


def bytes_v2(table, win):
    bx0, by0, bx1, by1 = block_range(win)
    ox, oy, rx, ry = (table[f].astype(np.int64) for f in ("ox", "oy", "rx", "ry"))
    iw = np.clip(np.minimum(ox + rx, bx1 + 1) - np.maximum(ox, bx0), 0, None)
    ih = np.clip(np.minimum(oy + ry, by1 + 1) - np.maximum(oy, by0), 0, None)
    blocks = (bx1 - bx0 + 1) * (by1 - by0 + 1)
    assert int((iw * ih).sum()) == blocks
    return {"table": 64 * len(table), "payload": int((iw * ih * field_bytes_per_block(table["shift"])).sum()), "stored": 4 * win[2] * win[3], "map": 12 * blocks}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default=None, help="workload:size, e.g. random_gradient:4096 (default: the two of the docstring)")
    args = ap.parse_args()
    assert args.reps >= 7 and args.warmup >= 2
    import torch
    import bench
    import limg_amd
    print(json.dumps(dict(tool="window_decode_bench", lib=os.path.basename(limg_amd.LIB_PATH), **bench.provenance())), flush=True)
    g = limg_amd.LimgHip(0)
    work = [("photo_noise", 8192), ("random_gradient", 4096)] if not args.only else [(args.only.split(":")[0], int(args.only.split(":")[1]))]
    for kind, n in work:
        img = g.synth_device(kind, n, n, seed=1)
        for version in (1, 2):
            if version == 1:
                st, nbytes = g.encode_stream_device(img, True)
                full, window = g.decode_stream_device, g.decode_stream_window_device
                table = st[64:64 + 56 * (n // 8) ** 2].cpu().numpy().view(limg_amd.STREAM_BLOCK_DTYPE)
                count = lambda win: bytes_v1(table, n // 8, win)  # noqa: E731
            else:
                st, nbytes = g.blocked_encode_stream_device(img, True)
                full, window = g.blocked_decode_stream_device, g.blocked_decode_stream_window_device
                rects = len(g.blocked_regions())
                table = st[64:64 + 64 * rects].cpu().numpy().view(limg_amd.STREAM_RECT_DTYPE)
                count = lambda win: bytes_v2(table, win)  # noqa: E731
            out_full = torch.empty((n, n), dtype=torch.int32, device="cuda")
            flat = torch.empty(1001 * 1000 + 8, dtype=torch.int32, device="cuda")
            wins = {"whole": (0, 0, n, n), "aligned": (1024, 2048, 1024, 1024), "unaligned": (123, 457, 1000, 1000)}
            calls = {
                "full": lambda: full(st, nbytes, n, n, out=out_full),
                "whole": lambda: window(st, nbytes, n, n, 0, 0, n, n, out=out_full, out_stride=n),
                "aligned": lambda: window(st, nbytes, n, n, *wins["aligned"], out=out_full, out_stride=1024),
                "unaligned": lambda: window(st, nbytes, n, n, *wins["unaligned"], out=flat[1:], out_stride=1001),
            }
            ms = {k: [] for k in calls}
            for rep in range(args.warmup + args.reps):
                for name, fn in calls.items():  # the variants alternate: same box, same clock
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    fn()
                    b.record()
                    torch.cuda.synchronize()
                    if rep >= args.warmup:
                        ms[name].append(a.elapsed_time(b))
            g.check()
            line = {"workload": kind, "size": n, "version": version, "stream_bytes": int(nbytes), "reps": args.reps}
            for name in calls:
                by = count(wins.get(name, wins["whole"]))
                total = sum(by.values())
                t = stats(ms[name])
                line[name] = {"ms": t, "bytes": by, "bytes_total": total, "share_of_hbm_peak": round(total / (t["median"] * 1e-3) / HBM_PEAK, 4)}
            line["whole_over_full"] = round(line["whole"]["ms"]["median"] / line["full"]["ms"]["median"], 3)
            print(json.dumps(line), flush=True)
            del st, out_full, flat
        del img
        torch.cuda.empty_cache()
    g.close()


if __name__ == "__main__":
    main()
