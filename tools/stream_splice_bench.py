#!/usr/bin/env python3
"""Timings of the stream splice (limg_hip_stream_splice_device / limg_hip_stream_crop_device) next to the only route a caller had without it -- decode the pixels,
encode them again -- and next to a plain device-to-device copy of the same byte count, through the ctypes view:

  python tools/stream_splice_bench.py [--reps 9] [--warmup 3] [--out profiles/stream_splice.md]

Cases (8192^2 photo-noise, synthesised and encoded on the device, RGBA):
  crop     the 1024^2 window at (3584, 3584) of the stream as a stream of its own
  tiles    the 4 x 4 tiling of the stream (16 crops of 2048^2, made before anything is timed) spliced back into the 8192^2 stream
  strips   16 strips of 8192 x 512, each encoded on its own (the ranks of a multi-GPU encode), joined into the 8192^2 stream
Variants, alternating within a repetition so that box and clock are shared:
  (a) re-encode  window decode of the source(s) into pixels, stream encode of the pixels.  LOSSY a second time: the dither chain restarts and the shift search runs
                 again on decoded pixels, so its result is another image than the source's; it is timed as the price of not having the splice, not as an equal
  (b) splice     ONE splice / crop call
  (c) copy       torch's copy_ of a contiguous uint8 tensor of the splice's output size (hipMemcpyAsync, device to device)
Before anything is timed the splice's output is decoded and compared, bit for bit, with the decode of its sources.  Each variant: HIP events on the launch stream
around all of its work, min / median / max in ms over the repetitions.  GB/s counts the bytes read plus written: twice the output's size, for the splice (every entry
and payload word is read once and written once; the measure pass reads another 8 of an entry's 56 bytes) and for the copy alike.  One JSON line per case; --out also
writes them as the profile's table.  Every comparison is reported, none is asserted."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 8192


def stats(v):
    v = sorted(v)
    return {"min": round(v[0], 4), "median": round(v[len(v) // 2], 4), "max": round(v[-1], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.reps >= 7 and args.warmup >= 2
    import torch
    import bench
    import limg_amd
    head = dict(tool="stream_splice_bench", lib=os.path.basename(limg_amd.LIB_PATH), **bench.provenance())
    print(json.dumps(head), flush=True)
    g = limg_amd.LimgHip(0)
    img = g.synth_device("photo_noise", N, N, seed=1)
    src, src_bytes = g.encode_stream_device(img, True)
    full = g.decode_stream_device(src, src_bytes, N, N)
    torch.cuda.synchronize()

    def event_clock(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        return lambda: a.elapsed_time(b)

    def crop_case():
        x = y = 3584
        out = torch.empty(g.stream_bound(1024, 1024), dtype=torch.uint8, device="cuda")
        px = torch.empty((1024, 1024), dtype=torch.int32, device="cuda")
        again = torch.empty_like(out)

        def splice():
            return g.stream_crop_device(src, src_bytes, N, N, True, x, y, 1024, 1024, 100, 1, out=out, want_size=False)

        def reencode():
            g.decode_stream_window_device(src, src_bytes, N, N, x, y, 1024, 1024, out=px)
            g.encode_stream_device(px, True, out=again, want_size=False)

        return "crop 1024^2 of 8192^2", 1, splice, reencode, out, (1024, 1024), full[y:y + 1024, x:x + 1024]

    def tiles_case():
        tiles = []
        for j in range(4):
            for i in range(4):
                t, n = g.stream_crop_device(src, src_bytes, N, N, True, 2048 * i, 2048 * j, 2048, 2048, 100, 1)
                tiles.append((t[:(n + 15) // 16 * 16].clone(), n, i, j))
        pieces = [((t, n), 0, 0, 256 * i, 256 * j, 256, 256, 2048, 2048) for t, n, i, j in tiles]
        out = torch.empty(g.stream_bound(N, N), dtype=torch.uint8, device="cuda")
        px = torch.empty((N, N), dtype=torch.int32, device="cuda")
        again = torch.empty_like(out)

        def splice():
            return g.stream_splice_device(pieces, N, N, True, 100, 1, out=out, want_size=False)

        def reencode():
            for t, n, i, j in tiles:
                g.decode_stream_window_device(t, n, 2048, 2048, 0, 0, 2048, 2048, out=px[2048 * j:, 2048 * i:], out_stride=N)
            g.encode_stream_device(px, True, out=again, want_size=False)

        return "4 x 4 tiles of 2048^2 -> 8192^2", 16, splice, reencode, out, (N, N), full

    def strips_case():
        strips, decoded = [], []
        for k in range(16):
            t, n = g.encode_stream_device(img[512 * k:512 * (k + 1)], True)
            strips.append((t[:(n + 15) // 16 * 16].clone(), n))
            decoded.append(g.decode_stream_device(t, n, N, 512))
        want = torch.cat(decoded)
        out = torch.empty(g.stream_bound(N, N), dtype=torch.uint8, device="cuda")
        px = torch.empty((N, N), dtype=torch.int32, device="cuda")
        again = torch.empty_like(out)

        pieces = [((t, n), 0, 0, 0, 64 * k, 1024, 64, N, 512) for k, (t, n) in enumerate(strips)]  # what join_strip_streams builds

        def splice():
            return g.stream_splice_device(pieces, N, N, True, 100, 1, out=out, want_size=False)

        def reencode():
            for k, (t, n) in enumerate(strips):
                g.decode_stream_device(t, n, N, 512, out=px[512 * k:512 * (k + 1)])
            g.encode_stream_device(px, True, out=again, want_size=False)

        return "16 strips of 8192 x 512 -> 8192^2", 16, splice, reencode, out, (N, N), want

    lines = []
    for case in (crop_case, tiles_case, strips_case):
        name, n_pieces, splice, reencode, out, (w, h), want = case()
        splice()
        torch.cuda.synchronize()
        g.check()
        out_bytes = int(out[:64].cpu().numpy().view(limg_amd.STREAM_HEADER_DTYPE)[0]["totalBytes"])
        got = g.decode_stream_device(out, out_bytes, w, h)
        torch.cuda.synchronize()
        lossless = bool(torch.equal(got, want))
        a, b = torch.empty(out_bytes, dtype=torch.uint8, device="cuda"), torch.empty(out_bytes, dtype=torch.uint8, device="cuda")
        copy = lambda: b.copy_(a)  # noqa: E731
        ms = {"reencode": [], "splice": [], "copy": []}
        for rep in range(args.warmup + args.reps):
            for variant, fn in (("reencode", reencode), ("splice", splice), ("copy", copy)):
                t = event_clock(fn)
                torch.cuda.synchronize()
                if rep >= args.warmup:
                    ms[variant].append(t())
        ms = {k: stats(v) for k, v in ms.items()}
        g.check()
        gbs = lambda s: round(2 * out_bytes / (s["median"] * 1e-3) / 1e9, 1)  # noqa: E731
        line = {"case": name, "pieces": n_pieces, "out_bytes": out_bytes, "reps": args.reps, "decode_equals_sources": lossless, "reencode_ms": ms["reencode"], "splice_ms": ms["splice"],
                "copy_ms": ms["copy"], "splice_gb_s": gbs(ms["splice"]), "copy_gb_s": gbs(ms["copy"]), "splice_over_copy": round(ms["splice"]["median"] / ms["copy"]["median"], 3),
                "reencode_over_splice": round(ms["reencode"]["median"] / ms["splice"]["median"], 2), "context_bytes": g.device_bytes()}
        print(json.dumps(line), flush=True)
        lines.append(line)
        del out, a, b, got, want
        torch.cuda.empty_cache()
    g.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("# Stream splice: crop and join of LMG3 streams by copying, against decode + encode and against a plain copy\n\n")
            f.write("Written by `tools/stream_splice_bench.py` (HIP events, %d warm-up + %d repetitions, the variants alternating in one process; times in ms as min / median / max).\n" % (args.warmup, args.reps))
            f.write("Re-encode: window decode of the source(s) into pixels, then stream encode of the pixels -- the only route without the splice, and LOSSY a second time (the dither\n")
            f.write("chain restarts, the shift search runs again), so it is the price of the missing feature and not an equal.  Splice: ONE call, three kernel launches.  Copy: a\n")
            f.write("device-to-device copy of the splice's output size.  GB/s: twice the output's size over the median time (bytes read plus written).\n\n")
            f.write("`%s`\n\n" % json.dumps(head))
            f.write("| case | pieces | output bytes | re-encode ms | splice ms | copy ms | splice GB/s | copy GB/s | splice / copy | re-encode / splice | decode(splice) == decode(sources) |\n")
            f.write("|---|---|---|---|---|---|---|---|---|---|---|\n")
            for ln in lines:
                fm = lambda s: "%.3f / %.3f / %.3f" % (s["min"], s["median"], s["max"])  # noqa: E731
                f.write("| %s | %d | %d | %s | %s | %s | %.1f | %.1f | %.3f | %.2f | %s |\n" % (ln["case"], ln["pieces"], ln["out_bytes"], fm(ln["reencode_ms"]), fm(ln["splice_ms"]), fm(ln["copy_ms"]),
                                                                                         ln["splice_gb_s"], ln["copy_gb_s"], ln["splice_over_copy"], ln["reencode_over_splice"],
                                                                                         ln["decode_equals_sources"]))


if __name__ == "__main__":
    main()
