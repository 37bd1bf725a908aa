#!/usr/bin/env python3
"""Timings of the stream error entries and of the stream encode to a quality target next to the existing entries they replace, through the ctypes view:

  python tools/stream_error_bench.py [--reps 20] [--warmup 3] [--out profiles/stream_error.md]

Three tables, every variant next to its yardstick in the same run, alternating within a repetition so that box and clock are shared; host clock around calls that
end in a wait for the device, ms, median (min - max) over the repetitions:
  1. error   one whole-image limg_hip_[blocked_]decode_stream_windows_error_device call and the download of its sum, against the pair it replaces:
             limg_hip_[blocked_]decode_stream_device into a full RGBA image + limg_hip_compare_device.  8192^2 photo-noise and 4096^2 gradient, both stream versions.
             Before anything is timed the two must give the same error sum.
  2. quality one limg_hip_encode_stream_quality_device call against the same search driven from Python over encode + decode + compare (the same probes).
  3. list    one limg_hip_encode_stream_quality_batch_device call against the loop of single quality calls, at 64 x 1024^2, 16 x 4096^2 and 4 x 8192^2 (search range
             [2, 128]).
One JSON line per row; --out also writes the tables as markdown."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(v):
    v = sorted(v)
    return {"min": round(v[0], 4), "median": round(v[len(v) // 2], 4), "max": round(v[-1], 4)}


def timed(variants, reps, warmup):
    """{name: fn} -> {name: stats of ms}; the variants alternate within a repetition"""
    import torch
    ms = {k: [] for k in variants}
    for rep in range(warmup + reps):
        for key, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rep >= warmup:
                ms[key].append((time.perf_counter() - t0) * 1e3)
    return {k: stats(v) for k, v in ms.items()}


def host_search(E, h_lo, h_hi, limit):
    """the algorithm of include/limg_hip.h ("stream encode to a quality target"); E(h) is asked once per value -> (h, within, last value asked, probes)"""
    memo, last = {}, [None]

    def e(h):
        if h not in memo:
            memo[h] = E(h)
            last[0] = h
        return memo[h]

    if e(h_lo) > limit:
        return h_lo, 0, last[0], len(memo)
    if e(h_hi) <= limit:
        return h_hi, 1, last[0], len(memo)
    lo, hi = h_lo, h_hi
    while hi - lo > 1:
        mid = hi - (hi - lo) // 2
        if e(mid) <= limit:
            lo = mid
        else:
            hi = mid
    return lo, 1, last[0], len(memo)


def fmt(s):
    return "%.3f (%.3f - %.3f)" % (s["median"], s["min"], s["max"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parts", default="1,2,3")
    args = ap.parse_args()
    assert args.reps >= 20 and args.warmup >= 2
    parts = {int(v) for v in args.parts.split(",")}
    import torch
    import bench
    import limg_amd
    head = dict(tool="stream_error_bench", lib=os.path.basename(limg_amd.LIB_PATH), **bench.provenance())
    print(json.dumps(head), flush=True)
    g = limg_amd.LimgHip(0)
    rows1, rows2, rows3 = [], [], []

    # ---- 1. the error call against decode + compare ----
    for kind, n in (("photo_noise", 8192), ("random_gradient", 4096)) if 1 in parts else ():
        img = g.synth_device(kind, n, n, seed=1)
        decoded = torch.empty((n, n), dtype=torch.int32, device="cuda")
        sums = torch.zeros(1, dtype=torch.int64, device="cuda")
        for version in (1, 2):
            blocked = version == 2
            st, nbytes = (g.blocked_encode_stream_device if blocked else g.encode_stream_device)(img, True)
            decode = g.blocked_decode_stream_device if blocked else g.decode_stream_device
            error = g.blocked_decode_stream_windows_error_device if blocked else g.decode_stream_windows_error_device
            job = [(st, nbytes, n, n, 0, 0, n, n, img, n)]

            def pair():
                decode(st, nbytes, n, n, out=decoded)
                return round(g.compare_device(img, decoded, True)[1] * n * n)

            def fused():
                error(job, sums=sums)
                return int(sums.cpu()[0])

            a, b = pair(), fused()
            g.check()
            assert a == b, ("the error call and decode + compare disagree", a, b)
            ms = timed({"pair": pair, "error": fused}, args.reps, args.warmup)
            spread = ms["pair"]["max"] - ms["pair"]["min"]
            row = {"table": 1, "kind": kind, "size": n, "version": version, "stream_bytes": nbytes, "bytes_per_pixel": round(nbytes / (n * n), 3), "error_sum": b, "reps": args.reps,
                   "pair_ms": ms["pair"], "error_ms": ms["error"], "pair_over_error": round(ms["pair"]["median"] / ms["error"]["median"], 3),
                   "error_not_slower_than_pair_plus_its_spread": ms["error"]["median"] <= ms["pair"]["median"] + spread}
            rows1.append(row)
            print(json.dumps(row), flush=True)
            del st
        del img, decoded
        torch.cuda.empty_cache()

    # ---- 2. the quality call against the search driven from Python ----
    for kind, n in (("photo_noise", 4096), ("random_gradient", 4096)) if 2 in parts else ():
        img = g.synth_device(kind, n, n, seed=1)
        decoded = torch.empty((n, n), dtype=torch.int32, device="cuda")
        outs = [torch.empty(g.stream_bound(n, n), dtype=torch.uint8, device="cuda") for _ in (0, 1)]

        def E(hh):
            _, nbytes = g.encode_stream_device(img, True, out=outs[0], error_factor=2 * hh)
            g.decode_stream_device(outs[0], nbytes, n, n, out=decoded)
            return round(g.compare_device(img, decoded, True)[1] * n * n)

        limit = (E(1) + E(512)) // 2

        def loop():
            h, within, last, probes = host_search(E, 1, 512, limit)
            if last != h:
                g.encode_stream_device(img, True, out=outs[0], error_factor=2 * h)
            return 2 * h, within, probes

        def call():
            _, res = g.encode_stream_quality_device(img, True, limit, out=outs[1])
            return res.errorFactor, res.withinTarget, res.probes, res.bytes

        a, b = loop(), call()
        g.check()
        assert a == b[:3], ("the call and the loop disagree", a, b)
        assert torch.equal(outs[0][:b[3]], outs[1][:b[3]]), "the call's stream is not the loop's"
        ms = timed({"loop": loop, "quality": call}, args.reps, args.warmup)
        row = {"table": 2, "kind": kind, "size": n, "limit": limit, "error_factor": b[0], "within": b[1], "probes": b[2], "bytes": b[3], "reps": args.reps, "loop_ms": ms["loop"],
               "quality_ms": ms["quality"], "loop_over_quality": round(ms["loop"]["median"] / ms["quality"]["median"], 3)}
        rows2.append(row)
        print(json.dumps(row), flush=True)
        del img, decoded, outs
        torch.cuda.empty_cache()

    # ---- 3. the list call against the loop of single calls ----
    for count, n in ((64, 1024), (16, 4096), (4, 8192)) if 3 in parts else ():
        imgs = [g.synth_device("photo_noise", n, n, seed=1 + k) for k in range(count)]
        outs = [[torch.empty(g.stream_bound(n, n), dtype=torch.uint8, device="cuda") for _ in range(count)] for _ in (0, 1)]
        limits = []
        for k, img in enumerate(imgs):  # half way between the errors at the bounds: E(hLo) is a refused search's error sum, E(hHi) that of a search any stream meets
            lo = g.encode_stream_quality_device(img, True, 0, 2, 128, out=outs[0][k])[1].errorSum
            hi = g.encode_stream_quality_device(img, True, 2 ** 63, 2, 128, out=outs[0][k])[1].errorSum
            limits.append((lo + hi) // 2)

        def loop():
            return [g.encode_stream_quality_device(img, True, lim, 2, 128, out=o)[1] for img, lim, o in zip(imgs, limits, outs[0])]

        def batch():
            return g.encode_stream_quality_batch_device(imgs, True, limits, 2, 128, outs=outs[1])[1]

        a, b = loop(), batch()
        g.check()
        key = lambda r: (r.errorFactor, r.withinTarget, r.probes, r.bytes, r.errorSum)  # noqa: E731
        assert [key(r) for r in a] == [key(r) for r in b], "the list call and the loop disagree"
        assert all(torch.equal(x[:r.bytes], y[:r.bytes]) for x, y, r in zip(outs[0], outs[1], b)), "the list call's streams are not the loop's"
        ms = timed({"loop": loop, "batch": batch}, args.reps, args.warmup)
        row = {"table": 3, "count": count, "size": n, "rounds": max(r.probes for r in b), "error_factors": sorted({r.errorFactor for r in b}), "reps": args.reps, "loop_ms": ms["loop"],
               "batch_ms": ms["batch"], "loop_over_batch": round(ms["loop"]["median"] / ms["batch"]["median"], 3)}
        rows3.append(row)
        print(json.dumps(row), flush=True)
        del imgs, outs
        torch.cuda.empty_cache()
    g.close()

    if args.out:
        with open(args.out, "w") as f:
            f.write("# Stream error inside the decode, and the stream encode to a quality target\n\n")
            f.write("Generated by `tools/stream_error_bench.py` (%d repetitions after %d warm-up runs, variants alternating; `%s`, head `%s`).  Host clock around calls that wait "
                    "for the device, ms, median (min - max).\n\n" % (args.reps, args.warmup, head["lib"], head.get("head", "?")))
            if rows1:
                f.write("## 1. One whole-image error call against decode + compare\n\n`pair`: `limg_hip_[blocked_]decode_stream_device` into a full RGBA image + "
                        "`limg_hip_compare_device`.  `error`: one `limg_hip_[blocked_]decode_stream_windows_error_device` over the window (0, 0, sizeX, sizeY) and the download of "
                        "its sum.  Both gave the same error sum (checked before timing).  The last column: the error call's median is no larger than the pair's median plus the "
                        "pair's own spread (max - min).\n\n")
                f.write("| image | version | stream B/px | pair ms | error ms | pair / error | not slower |\n|---|---|---|---|---|---|---|\n")
                for r in rows1:
                    f.write("| %s %d^2 | %d | %.3f | %s | %s | %.2f | %s |\n" % (r["kind"], r["size"], r["version"], r["bytes_per_pixel"], fmt(r["pair_ms"]), fmt(r["error_ms"]),
                                                                            r["pair_over_error"], "yes" if r["error_not_slower_than_pair_plus_its_spread"] else "NO"))
                f.write("\n")
            if rows2:
                f.write("## 2. One quality call against the search driven from Python\n\nSquare RGBA images; the limit half way between the error sums at errorFactor 2 and 1024; the "
                        "default search range.  `loop`: `limg_hip_encode_stream_device` + `limg_hip_decode_stream_device` + `limg_hip_compare_device` per probe, the same probes "
                        "as the call, and one more encode where the last probe was not the result.  `quality`: one `limg_hip_encode_stream_quality_device`.  Both chose the same "
                        "error factor and wrote the same stream (checked before timing).\n\n")
                f.write("| image | chosen errorFactor | probes | bytes | loop ms | quality ms | loop / quality |\n|---|---|---|---|---|---|---|\n")
                for r in rows2:
                    f.write("| %s %d^2 | %d | %d | %d | %s | %s | %.2f |\n" % (r["kind"], r["size"], r["error_factor"], r["probes"], r["bytes"], fmt(r["loop_ms"]), fmt(r["quality_ms"]),
                                                                          r["loop_over_quality"]))
                f.write("\n")
            if rows3:
                f.write("## 3. One list call against the loop of single quality calls\n\nPhoto-noise RGBA images of different seeds; every image's limit half way between its error sums "
                        "at errorFactor 2 and 128; search range [2, 128].  `loop`: one `limg_hip_encode_stream_quality_device` per image.  `batch`: one "
                        "`limg_hip_encode_stream_quality_batch_device`.  The same results and streams (checked before timing).  A ratio below 1 is a row where batching does not "
                        "pay.\n\n")
                f.write("| list | rounds | chosen errorFactors | loop ms | batch ms | loop / batch |\n|---|---|---|---|---|---|\n")
                for r in rows3:
                    f.write("| %d x %d^2 | %d | %s | %s | %s | %.2f |\n" % (r["count"], r["size"], r["rounds"], ", ".join(str(e) for e in r["error_factors"]), fmt(r["loop_ms"]),
                                                                        fmt(r["batch_ms"]), r["loop_over_batch"]))
                f.write("\n")


if __name__ == "__main__":
    main()
