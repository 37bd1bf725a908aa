#!/usr/bin/env python3
"""Timings of the budgeted stream encode of a LIST next to the loop of single budget calls it replaces, through the ctypes view:

  python tools/stream_budget_batch_bench.py [--reps 7] [--warmup 2] [--lists p1024,p4096,p8192] [--out profiles/stream_budget_batch.md] [--no-trace]

Lists (synthesised on the device, RGBA photo-noise, a different seed per image): p1024 = 64 x 1024^2, p4096 = 16 x 4096^2, p8192 = 4 x 8192^2.  The budget of an image
is 60 % of its size at errorFactor 2; the default search range [2, 1024].
Variants, alternating within a repetition so that box and clock are shared, both from device-resident images:
  (a) loop     limg_hip_encode_stream_budget_device once per image: per image the float stage, up to 11 probe / step pairs, a wait, a stream encode.  This is code the
               list entry does not touch -- the single call's kernels are what they were before it existed -- so it is the yardstick.
  (b) batched  ONE call of limg_hip_encode_stream_budget_batch_device
Both wait inside, so the clock is the host's around the call(s): min / median / max in ms over the repetitions.  Before anything is timed the two must agree on every
image's result and stream.  Also recorded: the distinct error factors of a list (= the final encodes the batched call makes: the thresholds are kernel arguments of the
encode kernel), and -- from a run of its own under `rocprofv3 --kernel-trace`, never together with counters -- the GPU time of every k_rate_probe_batch launch of one
call, early ones with every image still searching and late ones with most of them done; and k_rate_probe_batch's resource usage from the compiler's remarks.

This program is the driver: every GPU step is a child process under its own `timeout` (--worker / --trace-worker below are those children).  One JSON line per list."""
import argparse
import csv
import glob
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LISTS = {"p1024": (1024, 64), "p4096": (4096, 16), "p8192": (8192, 4)}
STEP_SECONDS = 240  # a worker's own time limit: synthesis + 2 x (warm-up + repetitions) of a few hundred ms


def stats(v):
    v = sorted(v)
    return {"min": round(v[0], 4), "median": round(v[len(v) // 2], 4), "max": round(v[-1], 4)}


def make_list(g, name):
    import torch
    n, count = LISTS[name]
    imgs = [g.synth_device("photo_noise", n, n, seed=1 + i) for i in range(count)]
    budgets = [int(0.6 * g.stream_sizes_device(img, True, [2])[0]) for img in imgs]
    outs = [[torch.empty(g.stream_bound(n, n), dtype=torch.uint8, device="cuda") for _ in range(count)] for _ in (0, 1)]
    return n, count, imgs, budgets, outs


def worker(name, reps, warmup):
    import torch
    import limg_amd
    g = limg_amd.LimgHip(0)
    n, count, imgs, budgets, outs = make_list(g, name)

    def loop():
        return [g.encode_stream_budget_device(img, True, b, out=o)[1] for img, b, o in zip(imgs, budgets, outs[0])]

    def batched():
        return g.encode_stream_budget_batch_device(imgs, True, budgets, outs=outs[1])[1]

    tup = lambda r: (r.errorFactor, r.withinBudget, r.probes, r.bytes)  # noqa: E731
    a, b = loop(), batched()
    torch.cuda.synchronize()
    g.check()
    assert [tup(r) for r in a] == [tup(r) for r in b], "the batched call and the loop disagree on a result"
    for x, y, r in zip(outs[0], outs[1], b):
        assert torch.equal(x[:r.bytes], y[:r.bytes]), "the batched call's stream is not the loop's"
    ms = {"loop": [], "batched": []}
    for rep in range(warmup + reps):
        for key, fn in (("loop", loop), ("batched", batched)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rep >= warmup:
                ms[key].append((time.perf_counter() - t0) * 1e3)
    g.check()
    ms = {k: stats(v) for k, v in ms.items()}
    efs = [r.errorFactor for r in b]
    print(json.dumps({"list": name, "size": n, "images": count, "reps": reps, "loop_ms": ms["loop"], "batched_ms": ms["batched"],
                      "loop_median_over_batched_median": round(ms["loop"]["median"] / ms["batched"]["median"], 3), "groups": len(set(efs)),
                      "error_factors": sorted(set(efs)), "probes": [r.probes for r in b], "met": sum(r.withinBudget for r in b), "stream_bytes": sum(r.bytes for r in b)}), flush=True)
    g.close()


def trace_worker(name):
    """what the kernel trace sees: two warm-up calls, then ONE batched call -- the trace's last launches of k_rate_probe_batch are that call's"""
    import torch
    import limg_amd
    g = limg_amd.LimgHip(0)
    _, _, imgs, budgets, outs = make_list(g, name)
    for _ in range(3):
        g.encode_stream_budget_batch_device(imgs, True, budgets, outs=outs[1])
        torch.cuda.synchronize()
    g.check()
    g.close()


def resource_usage():
    """the compiler's kernel-resource-usage remarks of limg_hip_rate.hip on the compile line that ships -> {kernel: {field: value}}"""
    from limg_amd import build
    with tempfile.TemporaryDirectory() as tmp:
        cmd = build.compile_line("limg_hip_rate.hip") + ["--cuda-device-only", "-c", os.path.join(build.CSRC, "limg_hip_rate.hip"), "-o", os.path.join(tmp, "rate.o"),
                                                          "-Rpass-analysis=kernel-resource-usage"]
        err = subprocess.run(cmd, capture_output=True, text=True).stderr
    out, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"remark:\s+(.*?):\s+(\S+) \[-Rpass-analysis", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = out.setdefault(subprocess.run(["c++filt", m.group(2)], capture_output=True, text=True).stdout.strip() or m.group(2), {})
        elif cur is not None:
            cur[m.group(1)] = m.group(2)
    return out


def run_step(cmd, seconds):
    """one child under its own time limit -> (its JSON lines, None) or ([], what went wrong)"""
    r = subprocess.run(["timeout", "-k", "10", str(seconds)] + cmd, capture_output=True, text=True, cwd=ROOT)
    if r.returncode != 0:
        return [], "exit status %d: %s" % (r.returncode, (r.stderr or r.stdout)[-400:].replace("\n", " | "))
    return [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")], None


def probe_trace(name, launches):
    """GPU ns of the last `launches` k_rate_probe_batch dispatches of a traced run, in launch order"""
    with tempfile.TemporaryDirectory() as tmp:
        _, err = run_step(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "-o", "trace", "--", sys.executable, os.path.abspath(__file__), "--trace-worker", name],
                          STEP_SECONDS)
        if err:
            return None, err
        rows = []
        for f in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                if "k_rate_probe_batch" in row.get("Kernel_Name", ""):
                    rows.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]) - int(row["Start_Timestamp"])))
    rows.sort()
    if len(rows) < launches:
        return None, "the trace holds %d launches of k_rate_probe_batch, %d expected" % (len(rows), launches)
    return [d for _, d in rows[-launches:]], None


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
    assert args.reps >= 7 and args.warmup >= 2
    if args.worker:
        return worker(args.worker, args.reps, args.warmup)
    if args.trace_worker:
        return trace_worker(args.trace_worker)
    import bench
    import limg_amd
    head = dict(tool="stream_budget_batch_bench", lib=os.path.basename(limg_amd.LIB_PATH), **bench.provenance())
    print(json.dumps(head), flush=True)
    rows, failed = [], []
    for name in args.lists.split(","):
        got, err = run_step([sys.executable, os.path.abspath(__file__), "--worker", name, "--reps", str(args.reps), "--warmup", str(args.warmup)], STEP_SECONDS)
        if err:
            failed.append((name, err))
            print(json.dumps({"list": name, "error": err}), flush=True)
            break  # nothing more is started on the GPU behind a step that failed
        rows += got
        print(json.dumps(got[-1]), flush=True)
    traces = {}
    if not args.no_trace and not failed:
        for name in [r["list"] for r in rows]:
            traces[name] = probe_trace(name, 11)  # rate_max_probes over [2, 1024]
            print(json.dumps({"list": name, "probe_launch_ns": traces[name][0], "trace_error": traces[name][1]}), flush=True)
            if traces[name][1]:
                break
    usage = {k: v for k, v in resource_usage().items() if "k_rate_probe" in k}
    print(json.dumps({"resource_usage": usage}), flush=True)
    if args.out:
        write_profile(args, head, rows, failed, traces, usage)


def write_profile(args, head, rows, failed, traces, usage):
    with open(args.out, "w") as f:
        first = next((r for r in rows if r["list"] == "p1024"), None)
        if first is None:
            f.write("**NOT MEASURED: the 64 x 1024^2 list did not run (%s).**\n\n" % (dict(failed).get("p1024", "not asked for")))
        elif first["batched_ms"]["median"] >= first["loop_ms"]["min"]:
            f.write("**ACCEPTANCE MISSED: at 64 x 1024^2 the batched call's median (%.3f ms) is not below the loop's minimum (%.3f ms).**\n\n" %
                    (first["batched_ms"]["median"], first["loop_ms"]["min"]))
        f.write("# Budgeted stream encode of a list: one call against the loop of single budget calls\n\n")
        f.write("Generated by `tools/stream_budget_batch_bench.py` (%d repetitions after %d warm-up runs, variants alternating, every list in a process of its own; `%s`, "
                "head `%s`).\n" % (args.reps, args.warmup, head["lib"], head.get("head", "?")))
        f.write("RGBA photo-noise synthesised on the device, a different seed per image; budget of an image = 60 % of its size at errorFactor 2; search range [2, 1024].  "
                "`loop`: `limg_hip_encode_stream_budget_device` once per image (existing code on the same build and box: the yardstick).  `batched`: one "
                "`limg_hip_encode_stream_budget_batch_device`.  Both from device-resident images, host clock around calls that wait for the device, ms, median (min - max).  "
                "The two agreed on every result and every stream before anything was timed.\n\n")
        f.write("| list | loop ms | batched ms | loop median / batched median | batched median < loop min | distinct error factors (final encodes) | budgets met |\n|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write("| %d x %d^2 | %.3f (%.3f - %.3f) | %.3f (%.3f - %.3f) | %.2f | %s | %d: %s | %d of %d |\n" %
                    (r["images"], r["size"], r["loop_ms"]["median"], r["loop_ms"]["min"], r["loop_ms"]["max"], r["batched_ms"]["median"], r["batched_ms"]["min"],
                     r["batched_ms"]["max"], r["loop_median_over_batched_median"], "yes" if r["batched_ms"]["median"] < r["loop_ms"]["min"] else "**no**", r["groups"],
                     ", ".join(str(e) for e in r["error_factors"]), r["met"], r["images"]))
        for name, err in failed:
            f.write("\nList `%s` did not run: %s.  Nothing was started behind it.\n" % (name, err))
        f.write("\n## GPU time of the probe launches of one batched call\n\n`rocprofv3 --kernel-trace` in a run of its own (no counters): the 11 launches of `k_rate_probe_batch` "
                "of one call, in launch order, microseconds.  Launch 1 measures every image at the upper bound, launch 2 at the lower bound; from launch 3 on an image whose "
                "search is over costs its workgroups one load each.\n\n")
        if not traces:
            f.write("Not collected in this run.\n")
        for r in rows:
            ns, err = traces.get(r["list"], (None, "not collected"))
            if ns is None:
                f.write("* %d x %d^2: no trace (%s)\n" % (r["images"], r["size"], err))
            else:
                f.write("* %d x %d^2 (probes per image: %d - %d): %s\n" % (r["images"], r["size"], min(r["probes"]), max(r["probes"]), ", ".join("%.1f" % (v / 1e3) for v in ns)))
        f.write("\n## Resource usage (compiler remarks, gfx950, the compile line that ships)\n\n| kernel | SGPRs | VGPRs | scratch bytes / lane | LDS bytes | occupancy waves / SIMD |\n|---|---|---|---|---|---|\n")
        for k in sorted(usage):
            u = usage[k]
            short = re.sub(r"^void limg_hip::\(anonymous namespace\)::", "", k).split("(")[0]
            f.write("| `%s` | %s | %s | %s | %s | %s |\n" % (short, u.get("TotalSGPRs"), u.get("VGPRs"), u.get("ScratchSize [bytes/lane]"), u.get("LDS Size [bytes/block]"),
                                                           u.get("Occupancy [waves/SIMD]")))


if __name__ == "__main__":
    main()
