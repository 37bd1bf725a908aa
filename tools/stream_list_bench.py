#!/usr/bin/env python3
"""Timings of the stream encode of a list of MIXED shapes (limg_hip_encode_stream_list_device) next to what a caller has without it, through the ctypes view:

  python tools/stream_list_bench.py [--reps 7] [--warmup 2] [--lists mixed64,mixed16,same64] [--out profiles/stream_list.md]

Lists (RGBA photo-noise synthesised on the device, seeded):
  mixed64  64 images, both sides drawn from the multiples of 8 in [256, 1536]
  mixed16  16 images, both sides drawn from the multiples of 8 in [2048, 4096]
  same64   64 x 1024^2, all one shape
Yardsticks on the same build, for the mixed lists: (a) `singles`, the loop of limg_hip_encode_stream_device calls; (b) `grouped`, the caller's best without the new
entry: group by shape, one limg_hip_encode_stream_batch_ef_device per group, the single call for a group of one.  For same64 the yardstick is
limg_hip_encode_stream_batch_ef_device itself, run TWICE per repetition, so that the spread it shows against itself stands next to the new entry's gap.
Error factors cycle through (20, 60, 100, 140).  Every call is asynchronous (no sizes asked for); the clock is a pair of HIP events on the stream around the call(s),
ending in a synchronise; every shape is warmed up first (the warm-up runs every variant), the variants alternate within a repetition: min / median / max in ms.
Before anything is timed the variants must agree on every stream.  From a run of its own under `rocprofv3 --kernel-trace --stats` (no counters): the GPU time of the
new route's launches for the mixed lists.

This program is the driver: every GPU step is a child process under its own `timeout` (--worker / --trace-worker below are those children).  One JSON line per list."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LISTS = {"mixed64": (64, 256, 1536, 11), "mixed16": (16, 2048, 4096, 12), "same64": (64, 1024, 1024, 13)}  # images, smallest side, largest side, seed
STEP_SECONDS = 400
FACTORS = (20, 60, 100, 140)
KERNELS = ("k_set_words", "k_fit_tpb_list", "k_encode_list_mixed", "k_stream_scan_strips_list", "k_stream_pack_strips_list")


def stats(v):
    v = sorted(v)
    return {"min": round(v[0], 4), "median": round(v[len(v) // 2], 4), "max": round(v[-1], 4)}


def shapes_of(name):
    import numpy as np
    count, lo, hi, seed = LISTS[name]
    rng = np.random.default_rng(seed)
    return [(int(w) * 8, int(h) * 8) for w, h in zip(rng.integers(lo // 8, hi // 8 + 1, count), rng.integers(lo // 8, hi // 8 + 1, count))]


def setup(name):
    import torch
    import limg_amd
    g = limg_amd.LimgHip(0)
    shapes = shapes_of(name)
    imgs = [g.synth_device("photo_noise", w, h, seed=1 + i) for i, (w, h) in enumerate(shapes)]
    efs = [FACTORS[i % len(FACTORS)] for i in range(len(shapes))]
    outs = [[torch.empty(g.stream_bound(w, h), dtype=torch.uint8, device="cuda") for w, h in shapes] for _ in range(3)]
    return g, shapes, imgs, efs, outs


def variants(g, shapes, imgs, efs, same):
    def listed(o):
        g.encode_stream_list_device(imgs, True, efs, outs=o, want_sizes=False)

    def singles(o):
        for i, img in enumerate(imgs):
            g.encode_stream_device(img, True, out=o[i], error_factor=efs[i], want_size=False)

    groups = {}
    for i, s in enumerate(shapes):
        groups.setdefault(s, []).append(i)

    def grouped(o):
        for idx in groups.values():
            if len(idx) == 1:
                g.encode_stream_device(imgs[idx[0]], True, out=o[idx[0]], error_factor=efs[idx[0]], want_size=False)
            else:
                g.encode_stream_batch_ef_device([imgs[i] for i in idx], True, [efs[i] for i in idx], outs=[o[i] for i in idx], want_sizes=False)

    def batch_ef(o):
        g.encode_stream_batch_ef_device(imgs, True, efs, outs=o, want_sizes=False)

    if same:
        return [("batch_ef", batch_ef, 1), ("list", listed, 0), ("batch_ef_again", batch_ef, 2)], len(groups)
    return [("singles", singles, 1), ("grouped", grouped, 2), ("list", listed, 0)], len(groups)


def worker(name, reps, warmup):
    import torch
    g, shapes, imgs, efs, outs = setup(name)
    same = name.startswith("same")
    var, distinct = variants(g, shapes, imgs, efs, same)
    for _, fn, k in var:
        fn(outs[k])
    torch.cuda.synchronize()
    g.check()
    for i in range(len(imgs)):
        total = int(outs[0][i][40:48].cpu().numpy().view("<u8")[0])  # the header's totalBytes
        assert torch.equal(outs[0][i][:total], outs[1][i][:total]) and torch.equal(outs[0][i][:total], outs[2][i][:total]), (name, i, "the routes' streams differ")
    ms = {tag: [] for tag, _, _ in var}
    for rep in range(warmup + reps):
        for tag, fn, k in var:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            fn(outs[k])
            b.record()
            torch.cuda.synchronize()
            if rep >= warmup:
                ms[tag].append(a.elapsed_time(b))
    g.check()
    pixels = sum(w * h for w, h in shapes)
    out = {"list": name, "images": len(shapes), "distinct_shapes": distinct, "pixels": pixels, "reps": reps, "ms": {t: stats(v) for t, v in ms.items()}}
    out["gpixel_s_list"] = round(pixels / out["ms"]["list"]["median"] / 1e6, 2)
    print(json.dumps(out), flush=True)
    g.close()


def trace_worker(name):
    """what the traced run executes: the new call three times (the first warms the shapes up)"""
    import torch
    g, shapes, imgs, efs, outs = setup(name)
    for _ in range(3):
        g.encode_stream_list_device(imgs, True, efs, outs=outs[0], want_sizes=False)
    torch.cuda.synchronize()
    g.check()
    g.close()


def run_step(cmd, seconds):
    """one child under its own time limit -> (its JSON lines, None) or ([], what went wrong)"""
    r = subprocess.run(["timeout", "-k", "10", str(seconds)] + cmd, capture_output=True, text=True, cwd=ROOT)
    if r.returncode != 0:
        return [], "exit status %d: %s" % (r.returncode, (r.stderr or r.stdout)[-400:].replace("\n", " | "))
    return [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")], None


def kernel_times(name):
    """{kernel: (calls, average ns)} of the new route's launches in a traced run of their own (three calls of the list entry)"""
    with tempfile.TemporaryDirectory() as tmp:
        _, err = run_step(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "trace", "--", sys.executable, os.path.abspath(__file__),
                           "--trace-worker", name], STEP_SECONDS)
        if err:
            return None, err
        got = {}
        for f in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                for k in KERNELS:
                    if k in row.get("Name", ""):
                        calls, total = got.get(k, (0, 0))
                        got[k] = (calls + int(row["Calls"]), total + int(row["TotalDurationNs"]))
    if not got:
        return None, "no launch of the new route in the trace"
    return {k: {"calls": c, "average_us": round(t / c / 1000.0, 2)} for k, (c, t) in got.items()}, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--lists", default=",".join(LISTS))
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--worker", default=None)
    ap.add_argument("--trace-worker", default=None)
    args = ap.parse_args()
    assert args.reps >= 5 and args.warmup >= 1
    if args.worker:
        return worker(args.worker, args.reps, args.warmup)
    if args.trace_worker:
        return trace_worker(args.trace_worker)
    import bench
    import limg_amd
    head = dict(tool="stream_list_bench", lib=os.path.basename(limg_amd.LIB_PATH), **bench.provenance())
    print(json.dumps(head), flush=True)
    lists, failed, traces = [], [], {}
    for name in args.lists.split(","):
        got, err = run_step([sys.executable, os.path.abspath(__file__), "--worker", name, "--reps", str(args.reps), "--warmup", str(args.warmup)], STEP_SECONDS)
        if err:
            failed.append((name, err))
            print(json.dumps({"list": name, "error": err}), flush=True)
            break  # nothing more is started on the GPU behind a step that failed
        lists += got
        print(json.dumps(got[-1]), flush=True)
    if not failed and not args.no_trace:
        for name in args.lists.split(","):
            if name.startswith("same"):
                continue
            t, err = kernel_times(name)
            print(json.dumps({"trace": name, "kernels": t, "error": err}), flush=True)
            if err:
                failed.append((name + " (trace)", err))
                break
            traces[name] = t
    if args.out:
        write_profile(args, head, lists, failed, traces)


def write_profile(args, head, lists, failed, traces):
    cell = lambda s: "%.3f (%.3f - %.3f)" % (s["median"], s["min"], s["max"])  # noqa: E731
    with open(args.out, "w") as f:
        f.write("# Stream encode of a list of mixed shapes: against the loop of single calls and against grouping by shape\n\n")
        f.write("Generated by `tools/stream_list_bench.py` (%d repetitions after %d warm-up runs of every variant, variants alternating, every list in a process of its own; `%s`, "
                "head `%s`).\n" % (args.reps, args.warmup, head["lib"], head.get("head", "?")))
        f.write("RGBA photo-noise synthesised on the device, seeded shapes, error factors cycling through %s.  All calls asynchronous from device-resident images, no sizes "
                "asked for; HIP events around the call(s), ending in a synchronise; ms, median (min - max).  The variants agreed on every stream before anything was "
                "timed.\n\n" % (FACTORS,))
        f.write("## 1. Mixed lists\n\n`singles`: the loop of `limg_hip_encode_stream_device`.  `grouped`: by shape, one `limg_hip_encode_stream_batch_ef_device` per group, the "
                "single call for a group of one.  `list`: one `limg_hip_encode_stream_list_device`.\n\n")
        f.write("| list | images | distinct shapes | Mpixel | singles ms | grouped ms | list ms | singles / list | grouped / list | list Gpixel/s |\n|---|---|---|---|---|---|---|---|---|---|\n")
        slower = []
        for l in lists:
            if "singles" not in l["ms"]:
                continue
            m = l["ms"]
            f.write("| %s | %d | %d | %.1f | %s | %s | %s | %.2f | %.2f | %.2f |\n" % (l["list"], l["images"], l["distinct_shapes"], l["pixels"] / 1e6, cell(m["singles"]), cell(m["grouped"]),
                                                                                 cell(m["list"]), m["singles"]["median"] / m["list"]["median"],
                                                                                 m["grouped"]["median"] / m["list"]["median"], l["gpixel_s_list"]))
            if m["list"]["median"] > m["grouped"]["median"]:
                slower.append(l["list"])
        f.write("\n" + ("The mixed call is SLOWER than grouping by shape on: %s (ratios below 1 in the table).\n" % ", ".join(slower) if slower else
                        "The mixed call is not slower than grouping by shape on any list of this run.\n"))
        f.write("\n## 2. A list of one shape through the new entry\n\nIt is handed to `limg_hip_encode_stream_batch_ef_device`'s route as it is.  The yardstick ran twice per "
                "repetition: `again` is its spread against itself.\n\n| list | batch_ef ms | batch_ef again ms | list ms | batch_ef / list | within batch_ef's own spread |\n|---|---|---|---|---|---|\n")
        for l in lists:
            if "batch_ef" not in l["ms"]:
                continue
            m = l["ms"]
            lo = min(m["batch_ef"]["min"], m["batch_ef_again"]["min"])
            hi = max(m["batch_ef"]["max"], m["batch_ef_again"]["max"])
            f.write("| %s | %s | %s | %s | %.3f | %s |\n" % (l["list"], cell(m["batch_ef"]), cell(m["batch_ef_again"]), cell(m["list"]), m["batch_ef"]["median"] / m["list"]["median"],
                                                         "yes" if lo <= m["list"]["median"] <= hi else "**no** (%.3f - %.3f)" % (lo, hi)))
        if traces:
            f.write("\n## 3. GPU time of the new route's launches\n\n`rocprofv3 --kernel-trace --stats` in a run of its own (no counters), three calls of the list entry: launches "
                    "and average microseconds per launch.  `k_set_words` is the table upload (3 KiB of kernel arguments per launch).\n\n| list | " + " | ".join("`%s`" % k for k in KERNELS) +
                    " |\n|---|" + "---|" * len(KERNELS) + "\n")
            for name, t in traces.items():
                f.write("| %s | " % name + " | ".join("%d x %.2f" % (t[k]["calls"], t[k]["average_us"]) if k in t else "-" for k in KERNELS) + " |\n")
        for name, err in failed:
            f.write("\nStep `%s` did not run: %s.  Nothing was started behind it.\n" % (name, err))


if __name__ == "__main__":
    main()
