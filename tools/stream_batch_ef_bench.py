#!/usr/bin/env python3
"""Timings of the batched stream encode with one error factor per image (limg_hip_encode_stream_batch_ef_device) next to what it replaces, through the ctypes view:

  python tools/stream_batch_ef_bench.py [--reps 7] [--warmup 2] [--lists p1024,p4096,p8192] [--out profiles/stream_batch_ef.md]

Lists (synthesised on the device, RGBA photo-noise, a different seed per image): p1024 = 64 x 1024^2, p4096 = 16 x 4096^2, p8192 = 4 x 8192^2.
1. The price of the table: the new call with ALL factors equal (100) against limg_hip_encode_stream_batch_device at that factor -- the existing kernel on the same build
   and box is the yardstick; the two differ in k_encode_list_rated / k_encode_persistent, one table launch per 64 images and one scalar load in the scan.
2. Against the alternative: lists with 2, 8 and all-distinct factors (never more than there are images) through the new call and through the GROUPED route -- one
   limg_hip_encode_stream_batch_device per factor that two or more images share, one limg_hip_encode_stream_device per factor of one image.
Every call is asynchronous (no sizes asked for); the clock is a pair of HIP events on the stream around the call(s), the variants alternating within a repetition:
min / median / max in ms.  Before anything is timed the variants of a row must agree on every stream.  Also recorded: the resource usage of the four
k_encode_list_rated instances and of their siblings k_encode_persistent<CH, FAST, true, false> from the compiler's remarks.

This program is the driver: every GPU step is a child process under its own `timeout` (--worker below is that child).  One JSON line per list."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LISTS = {"p1024": (1024, 64), "p4096": (4096, 16), "p8192": (8192, 4)}
STEP_SECONDS = 300  # a worker's own time limit: synthesis + 4 rows x 2 variants x (warm-up + repetitions) of tens of ms
SHARED = 100


def stats(v):
    v = sorted(v)
    return {"min": round(v[0], 4), "median": round(v[len(v) // 2], 4), "max": round(v[-1], 4)}


def factors(count, distinct):
    """`count` factors with `distinct` different values, 20, 60, 100, ...: image i takes value i % distinct"""
    return [20 + 40 * (i % distinct) for i in range(count)]


def worker(name, reps, warmup):
    import torch
    import limg_amd
    g = limg_amd.LimgHip(0)
    n, count = LISTS[name]
    imgs = [g.synth_device("photo_noise", n, n, seed=1 + i) for i in range(count)]
    outs = [[torch.empty(g.stream_bound(n, n), dtype=torch.uint8, device="cuda") for _ in range(count)] for _ in (0, 1)]

    def rated(efs, o):
        g.encode_stream_batch_ef_device(imgs, True, efs, outs=o, want_sizes=False)

    def shared(efs, o):
        g.encode_stream_batch_device(imgs, True, outs=o, want_sizes=False, error_factor=efs[0])

    def grouped(efs, o):
        for ef in sorted(set(efs)):
            idx = [i for i, e in enumerate(efs) if e == ef]
            if len(idx) == 1:
                g.encode_stream_device(imgs[idx[0]], True, out=o[idx[0]], error_factor=ef, want_size=False)
            else:
                g.encode_stream_batch_device([imgs[i] for i in idx], True, outs=[o[i] for i in idx], want_sizes=False, error_factor=ef)

    rows = [("table", [SHARED] * count, shared)]
    for d in (2, 8, count):
        if d <= count and not any(r[0] == "distinct_%d" % d for r in rows):
            rows.append(("distinct_%d" % d, factors(count, d), grouped))
    result = {"list": name, "size": n, "images": count, "reps": reps, "rows": []}
    for tag, efs, other in rows:
        rated(efs, outs[0]); other(efs, outs[1])
        torch.cuda.synchronize()
        g.check()
        for i, (x, y) in enumerate(zip(outs[0], outs[1])):
            total = int(x[40:48].cpu().numpy().view("<u8")[0])  # the header's totalBytes
            assert torch.equal(x[:total], y[:total]), (tag, i, "the new call's stream is not the other route's")
        ms = {"rated": [], "other": []}
        for rep in range(warmup + reps):
            for key, fn, o in (("other", other, outs[1]), ("rated", rated, outs[0])):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                fn(efs, o)
                b.record()
                torch.cuda.synchronize()
                if rep >= warmup:
                    ms[key].append(a.elapsed_time(b))
        g.check()
        r, o = stats(ms["rated"]), stats(ms["other"])
        result["rows"].append({"row": tag, "distinct": len(set(efs)), "rated_ms": r, "other_ms": o, "other_median_over_rated_median": round(o["median"] / r["median"], 3),
                               "gpixel_s_rated": round(count * n * n / r["median"] / 1e6, 2)})
    print(json.dumps(result), flush=True)
    g.close()


def resource_usage():
    """the compiler's kernel-resource-usage remarks of limg_hip_kernels.hip on the compile line that ships -> {kernel: {field: value}}"""
    from limg_amd import build
    with tempfile.TemporaryDirectory() as tmp:
        cmd = build.compile_line("limg_hip_kernels.hip") + ["--cuda-device-only", "-c", os.path.join(build.CSRC, "limg_hip_kernels.hip"), "-o", os.path.join(tmp, "k.o"),
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--lists", default=",".join(LISTS))
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", default=None)
    args = ap.parse_args()
    assert args.reps >= 7 and args.warmup >= 2
    if args.worker:
        return worker(args.worker, args.reps, args.warmup)
    import bench
    import limg_amd
    head = dict(tool="stream_batch_ef_bench", lib=os.path.basename(limg_amd.LIB_PATH), **bench.provenance())
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
    usage = {k: v for k, v in resource_usage().items() if "k_encode_list_rated" in k or re.search(r"k_encode_persistent<\d, (true|false), true, false>", k)}
    print(json.dumps({"resource_usage": usage}), flush=True)
    if args.out:
        write_profile(args, head, lists, failed, usage)


def write_profile(args, head, lists, failed, usage):
    cell = lambda s: "%.3f (%.3f - %.3f)" % (s["median"], s["min"], s["max"])  # noqa: E731
    with open(args.out, "w") as f:
        f.write("# Batched stream encode with one error factor per image: the price of the table, and the grouped route it replaces\n\n")
        f.write("Generated by `tools/stream_batch_ef_bench.py` (%d repetitions after %d warm-up runs, variants alternating, every list in a process of its own; `%s`, head `%s`).\n"
                % (args.reps, args.warmup, head["lib"], head.get("head", "?")))
        f.write("RGBA photo-noise synthesised on the device, a different seed per image.  All calls asynchronous from device-resident images, no sizes asked for; HIP events "
                "around the call(s), ms, median (min - max).  The variants of a row agreed on every stream before anything was timed.\n\n")
        f.write("## 1. The price of the table: all factors equal (%d)\n\n`shared`: `limg_hip_encode_stream_batch_device` (k_encode_persistent, thresholds in kernel arguments) -- "
                "the yardstick.  `per image`: `limg_hip_encode_stream_batch_ef_device` (k_encode_list_rated, thresholds from the device table).\n\n" % SHARED)
        f.write("| list | shared ms | per image ms | shared median / per-image median | gap beyond the shared call's spread |\n|---|---|---|---|---|\n")
        for l in lists:
            r = next(x for x in l["rows"] if x["row"] == "table")
            beyond = r["rated_ms"]["median"] > r["other_ms"]["max"] or r["rated_ms"]["median"] < r["other_ms"]["min"]
            f.write("| %d x %d^2 | %s | %s | %.3f | %s |\n" % (l["images"], l["size"], cell(r["other_ms"]), cell(r["rated_ms"]), r["other_median_over_rated_median"],
                                                            "**yes** (%+.3f ms)" % (r["rated_ms"]["median"] - r["other_ms"]["median"]) if beyond else "no"))
        f.write("\n## 2. Against the grouped route\n\n`grouped`: one `limg_hip_encode_stream_batch_device` per factor that two or more images share, one "
                "`limg_hip_encode_stream_device` per factor of one image.  `per image`: one `limg_hip_encode_stream_batch_ef_device`.\n\n")
        f.write("| list | distinct factors | grouped ms | per image ms | grouped median / per-image median | per image Gpixel/s |\n|---|---|---|---|---|---|\n")
        for l in lists:
            for r in l["rows"]:
                if r["row"] != "table":
                    f.write("| %d x %d^2 | %d | %s | %s | %.2f | %.2f |\n" % (l["images"], l["size"], r["distinct"], cell(r["other_ms"]), cell(r["rated_ms"]),
                                                                             r["other_median_over_rated_median"], r["gpixel_s_rated"]))
        for name, err in failed:
            f.write("\nList `%s` did not run: %s.  Nothing was started behind it.\n" % (name, err))
        f.write("\n## Resource usage (compiler remarks, gfx950, the compile line that ships)\n\n| kernel | SGPRs | VGPRs | scratch bytes / lane | LDS bytes | occupancy waves / SIMD |\n|---|---|---|---|---|---|\n")
        for k in sorted(usage):
            u = usage[k]
            short = re.sub(r"^void limg_hip::\(anonymous namespace\)::", "", k).split("(")[0]
            f.write("| `%s` | %s | %s | %s | %s | %s |\n" % (short, u.get("TotalSGPRs"), u.get("VGPRs"), u.get("ScratchSize [bytes/lane]"), u.get("LDS Size [bytes/block]"),
                                                           u.get("Occupancy [waves/SIMD]")))


if __name__ == "__main__":
    main()
