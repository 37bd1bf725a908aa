#!/usr/bin/env python3
"""Timings of the budgeted stream encode of a list of MIXED shapes (limg_hip_encode_stream_budget_list_device) next to what a caller has without it, through the
ctypes view:

  python tools/stream_budget_list_bench.py [--reps 7] [--warmup 2] [--lists mixed64,mixed16,same64] [--out profiles/stream_budget_list.md]

Lists (RGBA photo-noise synthesised on the device, seeded; the shapes of tools/stream_list_bench.py):
  mixed64  64 images, both sides drawn from the multiples of 8 in [256, 1536]
  mixed16  16 images, both sides drawn from the multiples of 8 in [2048, 4096]
  same64   64 x 1024^2, all one shape
Every image's budget is 0.6 x its size at error factor 2 (from limg_hip_stream_sizes_list_device, whose one call is timed too); the bounds are the defaults [2, 1024].
Yardsticks on the same build, for the mixed lists: (a) `singles`, the loop of limg_hip_encode_stream_budget_device calls; (b) `grouped`, the caller's best without
the new entry: group by shape, one limg_hip_encode_stream_budget_batch_device per group, the single call for a group of one.  For same64 the yardstick is
limg_hip_encode_stream_budget_batch_device itself, run TWICE per repetition, so that the spread it shows against itself stands next to the new entry's gap.
Every call waits for its search states, so it is synchronous by nature; the clock is a pair of HIP events on the stream around the call(s), ending in a synchronise;
every shape is warmed up first (the warm-up runs every variant), the variants alternate within a repetition: min / median / max in ms.  Before anything is timed the
variants must agree on every result and every stream.  No ratio is a pass condition.

This program is the driver: every GPU step is a child process under its own `timeout` (--worker below is that child).  One JSON line per list."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LISTS = {"mixed64": (64, 256, 1536, 11), "mixed16": (16, 2048, 4096, 12), "same64": (64, 1024, 1024, 13)}  # images, smallest side, largest side, seed
STEP_SECONDS = 400


def stats(v):
    v = sorted(v)
    return {"min": round(v[0], 4), "median": round(v[len(v) // 2], 4), "max": round(v[-1], 4)}


def shapes_of(name):
    import numpy as np
    count, lo, hi, seed = LISTS[name]
    rng = np.random.default_rng(seed)
    return [(int(w) * 8, int(h) * 8) for w, h in zip(rng.integers(lo // 8, hi // 8 + 1, count), rng.integers(lo // 8, hi // 8 + 1, count))]


def variants(g, shapes, imgs, budgets, same):
    def listed(o):
        return g.encode_stream_budget_list_device(imgs, True, budgets, outs=o)[1]

    def singles(o):
        return [g.encode_stream_budget_device(img, True, budgets[i], out=o[i])[1] for i, img in enumerate(imgs)]

    groups = {}
    for i, s in enumerate(shapes):
        groups.setdefault(s, []).append(i)

    def grouped(o):
        res = [None] * len(imgs)
        for idx in groups.values():
            if len(idx) == 1:
                res[idx[0]] = g.encode_stream_budget_device(imgs[idx[0]], True, budgets[idx[0]], out=o[idx[0]])[1]
            else:
                for i, r in zip(idx, g.encode_stream_budget_batch_device([imgs[i] for i in idx], True, [budgets[i] for i in idx], outs=[o[i] for i in idx])[1]):
                    res[i] = r
        return res

    def budget_batch(o):
        return g.encode_stream_budget_batch_device(imgs, True, budgets, outs=o)[1]

    if same:
        return [("budget_batch", budget_batch, 1), ("list", listed, 0), ("budget_batch_again", budget_batch, 2)], len(groups)
    return [("singles", singles, 1), ("grouped", grouped, 2), ("list", listed, 0)], len(groups)


def worker(name, reps, warmup):
    import torch
    import limg_amd
    g = limg_amd.LimgHip(0)
    shapes = shapes_of(name)
    imgs = [g.synth_device("photo_noise", w, h, seed=1 + i) for i, (w, h) in enumerate(shapes)]
    outs = [[torch.empty(g.stream_bound(w, h), dtype=torch.uint8, device="cuda") for w, h in shapes] for _ in range(3)]
    budgets = [int(0.6 * int(v)) for v in g.stream_sizes_list_device(imgs, True, [2])[:, 0]]
    same = name.startswith("same")
    var, distinct = variants(g, shapes, imgs, budgets, same)
    tup = lambda r: (r.errorFactor, r.withinBudget, r.probes, r.bytes)  # noqa: E731
    first = {k: [tup(r) for r in fn(outs[k])] for _, fn, k in var}
    torch.cuda.synchronize()
    g.check()
    assert first[0] == first[1] == first[2], (name, "the routes' results differ")
    for i in range(len(imgs)):
        total = first[0][i][3]
        assert torch.equal(outs[0][i][:total], outs[1][i][:total]) and torch.equal(outs[0][i][:total], outs[2][i][:total]), (name, i, "the routes' streams differ")
    var.append(("sizes_list_1", lambda o: g.stream_sizes_list_device(imgs, True, [2]), 0))
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
    out = {"list": name, "images": len(shapes), "distinct_shapes": distinct, "pixels": pixels, "reps": reps, "ms": {t: stats(v) for t, v in ms.items()},
           "within_budget": sum(r[1] for r in first[0]), "probes": sum(r[2] for r in first[0]), "most_probes": max(r[2] for r in first[0])}
    print(json.dumps(out), flush=True)
    g.close()


def run_step(cmd, seconds):
    """one child under its own time limit -> (its JSON lines, None) or ([], what went wrong)"""
    r = subprocess.run(["timeout", "-k", "10", str(seconds)] + cmd, capture_output=True, text=True, cwd=ROOT)
    if r.returncode != 0:
        return [], "exit status %d: %s" % (r.returncode, (r.stderr or r.stdout)[-400:].replace("\n", " | "))
    return [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")], None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--lists", default=",".join(LISTS))
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", default=None)
    args = ap.parse_args()
    assert args.reps >= 5 and args.warmup >= 1
    if args.worker:
        return worker(args.worker, args.reps, args.warmup)
    import bench
    import limg_amd
    head = dict(tool="stream_budget_list_bench", lib=os.path.basename(limg_amd.LIB_PATH), **bench.provenance())
    print(json.dumps(head), flush=True)
    lists, failed = [], []
    for name in args.lists.split(","):
        got, err = run_step([sys.executable, os.path.abspath(__file__), "--worker", name, "--reps", str(args.reps), "--warmup", str(args.warmup)], STEP_SECONDS)
        if err:
            failed.append((name, err))
            print(json.dumps({"list": name, "error": err}), flush=True)
            break  # nothing more is started on the GPU behind a step that failed
        lists += got
        print(json.dumps(got[-1]), flush=True)
    if args.out:
        write_profile(args, head, lists, failed)


def write_profile(args, head, lists, failed):
    cell = lambda s: "%.3f (%.3f - %.3f)" % (s["median"], s["min"], s["max"])  # noqa: E731
    with open(args.out, "w") as f:
        f.write("# Budgeted stream encode of a list of mixed shapes: against the loop of single budget calls and against grouping by shape\n\n")
        f.write("Generated by `tools/stream_budget_list_bench.py` (%d repetitions after %d warm-up runs of every variant, variants alternating, every list in a process of its "
                "own; `%s`, head `%s`).\n" % (args.reps, args.warmup, head["lib"], head.get("head", "?")))
        f.write("RGBA photo-noise synthesised on the device, seeded shapes, every image's budget 0.6 x its size at error factor 2, the default bounds [2, 1024].  "
                "Device-resident images; HIP events around the call(s), ending in a synchronise; ms, median (min - max).  The variants agreed on every result and every "
                "stream before anything was timed.  One run on one machine; no ratio is a pass condition.\n\n")
        f.write("## 1. Mixed lists\n\n`singles`: the loop of `limg_hip_encode_stream_budget_device`.  `grouped`: by shape, one `limg_hip_encode_stream_budget_batch_device` per "
                "group, the single call for a group of one.  `list`: one `limg_hip_encode_stream_budget_list_device`.  `sizes`: one `limg_hip_stream_sizes_list_device` with "
                "one factor (the float stage, one probe, one download).\n\n")
        f.write("| list | images | distinct shapes | Mpixel | within budget | probes (most) | singles ms | grouped ms | list ms | singles / list | grouped / list | sizes ms |\n"
                "|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        slower = []
        for l in lists:
            if "singles" not in l["ms"]:
                continue
            m = l["ms"]
            f.write("| %s | %d | %d | %.1f | %d | %d (%d) | %s | %s | %s | %.2f | %.2f | %s |\n" % (
                l["list"], l["images"], l["distinct_shapes"], l["pixels"] / 1e6, l["within_budget"], l["probes"], l["most_probes"], cell(m["singles"]), cell(m["grouped"]),
                cell(m["list"]), m["singles"]["median"] / m["list"]["median"], m["grouped"]["median"] / m["list"]["median"], cell(m["sizes_list_1"])))
            if m["list"]["median"] > m["grouped"]["median"]:
                slower.append(l["list"])
        f.write("\n" + ("The list call is SLOWER than grouping by shape on: %s (ratios below 1 in the table).\n" % ", ".join(slower) if slower else
                        "The list call is not slower than grouping by shape on any list of this run.\n"))
        f.write("\n## 2. A list of one shape through the new entry\n\nIt is handed to `limg_hip_encode_stream_budget_batch_device`'s route as it is.  The yardstick ran twice "
                "per repetition: `again` is its spread against itself.\n\n| list | budget_batch ms | budget_batch again ms | list ms | budget_batch / list | within budget_batch's "
                "own spread |\n|---|---|---|---|---|---|\n")
        for l in lists:
            if "budget_batch" not in l["ms"]:
                continue
            m = l["ms"]
            lo = min(m["budget_batch"]["min"], m["budget_batch_again"]["min"])
            hi = max(m["budget_batch"]["max"], m["budget_batch_again"]["max"])
            f.write("| %s | %s | %s | %s | %.3f | %s |\n" % (l["list"], cell(m["budget_batch"]), cell(m["budget_batch_again"]), cell(m["list"]),
                                                         m["budget_batch"]["median"] / m["list"]["median"],
                                                         "yes" if lo <= m["list"]["median"] <= hi else "**no** (%.3f - %.3f)" % (lo, hi)))
        for name, err in failed:
            f.write("\nStep `%s` did not run: %s.  Nothing was started behind it.\n" % (name, err))


if __name__ == "__main__":
    main()
