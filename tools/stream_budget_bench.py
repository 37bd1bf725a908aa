#!/usr/bin/env python3
"""Timings of the budgeted stream encode next to the host-side search it replaces, through the ctypes view:

  python tools/stream_budget_bench.py [--reps 7] [--warmup 2] [--sizes 1024,4096,8192] [--out profiles/stream_budget.md]

Rows: square RGBA images synthesised on the device, photo-noise and random-gradient, the budget at 60 % of the stream's size at errorFactor 2, the default search
range [2, 1024].  Variants, alternating within a repetition so that box and clock are shared:
  (a) loop    what a caller had before: limg_hip_encode_stream_device with its size read back, once per probe, driven by the search of include/limg_hip.h restated
              here in Python -- so both variants make the same probes -- and once more at the result unless the last probe was the result
  (b) budget  ONE call of limg_hip_encode_stream_budget_device: the float stage once, a size probe per step, one wait, one stream encode
Both are timed by a host clock around calls that end in a wait for the device (each variant waits inside), min / median / max in ms over the repetitions.  Before
anything is timed the two must choose the same error factor and produce the same stream.  Per-probe GPU time (HIP events): limg_hip_stream_sizes_device with 17 and
with 1 entries at the chosen error factor, the difference over 16 (k_rate_probe + k_rate_step), next to one limg_hip_encode_stream_device without the size.
One JSON line per row; --out also writes the table as markdown."""
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


def host_search(size, h_lo, h_hi, budget):
    """the algorithm of include/limg_hip.h; size(h) is asked once per value -> (h, within, last value asked)"""
    memo, last = {}, [None]

    def sz(h):
        if h not in memo:
            memo[h] = size(h)
            last[0] = h
        return memo[h]

    if sz(h_hi) > budget:
        return h_hi, 0, last[0], len(memo)
    if sz(h_lo) <= budget:
        return h_lo, 1, last[0], len(memo)
    lo, hi = h_lo, h_hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if sz(mid) <= budget:
            hi = mid
        else:
            lo = mid
    return hi, 1, last[0], len(memo)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="1024,4096,8192")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.reps >= 7 and args.warmup >= 2
    import torch
    import bench
    import limg_amd
    head = dict(tool="stream_budget_bench", lib=os.path.basename(limg_amd.LIB_PATH), **bench.provenance())
    print(json.dumps(head), flush=True)
    g = limg_amd.LimgHip(0)
    rows = []
    for n in (int(v) for v in args.sizes.split(",")):
        for kind in ("photo_noise", "random_gradient"):
            img = g.synth_device(kind, n, n, seed=1)
            outs = [torch.empty(g.stream_bound(n, n), dtype=torch.uint8, device="cuda") for _ in (0, 1)]
            budget = int(0.6 * g.stream_sizes_device(img, True, [2])[0])

            def loop():
                h, within, last, probes = host_search(lambda hh: g.encode_stream_device(img, True, out=outs[0], error_factor=2 * hh)[1], 1, 512, budget)
                nbytes = g.encode_stream_device(img, True, out=outs[0], error_factor=2 * h)[1] if last != h else None
                return 2 * h, within, probes, nbytes

            def budgeted():
                _, res = g.encode_stream_budget_device(img, True, budget, out=outs[1])
                return res.errorFactor, res.withinBudget, res.probes, res.bytes

            a, b = loop(), budgeted()
            g.check()
            assert a[:3] == b[:3], ("the call and the loop disagree", a, b)
            assert torch.equal(outs[0][:b[3]], outs[1][:b[3]]), "the call's stream is not the loop's"
            ms = {"loop": [], "budget": []}
            for rep in range(args.warmup + args.reps):
                for key, fn in (("loop", loop), ("budget", budgeted)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    if rep >= args.warmup:
                        ms[key].append((time.perf_counter() - t0) * 1e3)
            # GPU time of one probe and of one whole stream encode at the chosen error factor
            ef = b[0]
            per = {"sizes17": [], "sizes1": [], "encode": []}
            for rep in range(args.warmup + args.reps):
                for key, fn in (("sizes17", lambda: g.stream_sizes_device(img, True, [ef] * 17)), ("sizes1", lambda: g.stream_sizes_device(img, True, [ef])),
                                ("encode", lambda: g.encode_stream_device(img, True, out=outs[0], error_factor=ef, want_size=False))):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    torch.cuda.synchronize()
                    if rep >= args.warmup:
                        per[key].append(e0.elapsed_time(e1))
            g.check()
            ms = {k: stats(v) for k, v in ms.items()}
            per = {k: stats(v) for k, v in per.items()}
            row = {"kind": kind, "size": n, "budget": budget, "error_factor": ef, "within": b[1], "probes": b[2], "bytes": b[3], "reps": args.reps, "loop_ms": ms["loop"],
                   "budget_ms": ms["budget"], "speedup_median": round(ms["loop"]["median"] / ms["budget"]["median"], 3),
                   "probe_gpu_ms": round((per["sizes17"]["median"] - per["sizes1"]["median"]) / 16, 4), "sizes1_gpu_ms": per["sizes1"], "sizes17_gpu_ms": per["sizes17"],
                   "encode_gpu_ms": per["encode"]}
            rows.append(row)
            print(json.dumps(row), flush=True)
            del img, outs
            torch.cuda.empty_cache()
    g.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("# Stream encode to a byte budget: one call against the host-side search it replaces\n\n")
            f.write("Generated by `tools/stream_budget_bench.py` (%d repetitions after %d warm-up runs, variants alternating; `%s`, head `%s`).\n" %
                    (args.reps, args.warmup, head["lib"], head.get("head", "?")))
            f.write("Square RGBA images synthesised on the device; budget = 60 % of the size at errorFactor 2; search range [2, 1024].  `loop`: "
                    "`limg_hip_encode_stream_device` with its size read back once per probe, the same probes as the call.  `budget`: one "
                    "`limg_hip_encode_stream_budget_device`.  Host clock around calls that wait for the device, ms, median (min - max).\n\n")
            f.write("| image | budget bytes | chosen errorFactor | probes | bytes | met | loop ms | budget ms | loop / budget |\n|---|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                f.write("| %s %d^2 | %d | %d | %d | %d | %s | %.3f (%.3f - %.3f) | %.3f (%.3f - %.3f) | %.2f |\n" %
                        (r["kind"], r["size"], r["budget"], r["error_factor"], r["probes"], r["bytes"], "yes" if r["within"] else "no", r["loop_ms"]["median"], r["loop_ms"]["min"],
                         r["loop_ms"]["max"], r["budget_ms"]["median"], r["budget_ms"]["min"], r["budget_ms"]["max"], r["speedup_median"]))
            f.write("\nThe call picked the same error factor as the loop on every row and wrote the same stream (checked before timing).\n\n")
            f.write("## GPU time per probe\n\nHIP events around `limg_hip_stream_sizes_device` with 17 entries and with 1 entry at the chosen error factor: the difference "
                    "over 16 is one `k_rate_probe` + `k_rate_step`; the 1-entry call is `k_fit_tpb` + one probe + the download.  Next to it one "
                    "`limg_hip_encode_stream_device` (no size read back) at the same error factor.  ms, median (min - max).\n\n")
            f.write("| image | per probe | sizes, 1 entry | stream encode | encode / probe |\n|---|---|---|---|---|\n")
            for r in rows:
                f.write("| %s %d^2 | %.4f | %.4f (%.4f - %.4f) | %.4f (%.4f - %.4f) | %.2f |\n" %
                        (r["kind"], r["size"], r["probe_gpu_ms"], r["sizes1_gpu_ms"]["median"], r["sizes1_gpu_ms"]["min"], r["sizes1_gpu_ms"]["max"], r["encode_gpu_ms"]["median"],
                         r["encode_gpu_ms"]["min"], r["encode_gpu_ms"]["max"], r["encode_gpu_ms"]["median"] / max(r["probe_gpu_ms"], 1e-9)))


if __name__ == "__main__":
    main()
