#!/usr/bin/env python3
"""Timings of the version 2 stream (merged-block encoder -> rectangles -> "LMG3" version 2) next to the plane encode and version 1, through the ctypes view:

  python tools/blocked_stream_bench.py [--size 8192] [--workload photo_noise] [--reps 7] [--warmup 2]

Per image it prints one JSON line: wall time (HIP events on the stream, host stages included: the entries return when everything is enqueued and the events bracket
the call) of blocked_encode3d_device and of blocked_encode_stream_device, min / median / max over the repetitions; the kernel-only sums of
limg_hip_blocked_kernel_timing for both (slot [3] holds the packer after a stream encode); pack-only time (limg_hip_blocked_last_stream's kernels, events),
decode time, the version 1 pack + decode on the same image, and the sizes of both streams.  Bytes moved are the algorithmic ones: pack reads the factor bytes of the
fields it writes and the noise bytes of the dithered ones and writes the stream; decode reads the stream and writes 4 B/px.  HBM peak: 8 TB/s (MI355X)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HBM_PEAK = 8.0e12


def stats(v):
    v = sorted(v)
    return {"min": round(v[0], 4), "median": round(v[len(v) // 2], 4), "max": round(v[-1], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--workload", default="photo_noise", choices=["photo_noise", "random_gradient"])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-planes", action="store_true", help="skip the plane encode (what the parent commit has: run it there with this tool's --planes-only)")
    ap.add_argument("--planes-only", action="store_true", help="time blocked_encode3d_device only (runs on a library without the stream entries)")
    args = ap.parse_args()
    import ctypes as C
    import torch
    import limg_amd
    g = limg_amd.LimgHip(0)
    n = args.size
    px = n * n
    img = g.synth_device(args.workload, n, n, seed=1)
    out = {"tool": "blocked_stream_bench", "size": n, "workload": args.workload, "reps": args.reps, "lib": os.path.basename(limg_amd.LIB_PATH)}

    def timed(fn, reps):
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return ms

    if not args.no_planes:
        planes = g.alloc_blocked_planes_device(n, n)
        enc = lambda: g.blocked_encode3d_device(img, True, planes)  # noqa: E731
        timed(enc, args.warmup)
        wall, kern = [], []
        for _ in range(args.reps):
            wall += timed(enc, 1)
            kern.append(sum(g.blocked_kernel_timing().values()))
        out["plane_encode_wall_ms"] = stats(wall)
        out["plane_encode_kernel_ms"] = stats(kern)
        out["plane_encode_kernel_slots_ms"] = {k: round(v, 4) for k, v in g.blocked_kernel_timing().items()}
        del planes
    if args.planes_only:
        print(json.dumps(out))
        return
    cap = g.blocked_stream_bound(n, n)
    st = torch.empty(cap, dtype=torch.uint8, device="cuda")
    enc = lambda: g.blocked_encode_stream_device(img, True, out=st, want_size=False)  # noqa: E731
    timed(enc, args.warmup)
    wall, kern = [], []
    for _ in range(args.reps):
        wall += timed(enc, 1)
        kern.append(sum(g.blocked_kernel_timing().values()))
    out["stream_encode_wall_ms"] = stats(wall)
    out["stream_encode_kernel_ms"] = stats(kern)
    out["stream_encode_kernel_slots_ms"] = {k: round(v, 4) for k, v in g.blocked_kernel_timing().items()}
    _, nbytes = g.blocked_encode_stream_device(img, True, out=st)
    regions = len(g.blocked_regions())
    # the packer alone: limg_hip_blocked_last_stream re-runs scan + pack over what the encode left in the context; its HIP events are added to slot [3] of the
    # kernel timing, so the slot's growth over one call is the packer's time
    pack = []
    for _ in range(args.reps + args.warmup):
        before = g.blocked_kernel_timing()["expand_store_kernels"]
        hb = np.zeros(cap, dtype=np.uint8)
        nb = C.c_size_t(0)
        r = g.lib.limg_hip_blocked_last_stream(g.ctx, hb.ctypes.data_as(C.c_void_p), cap, C.byref(nb))
        assert r == 0 and nb.value == nbytes
        pack.append(g.blocked_kernel_timing()["expand_store_kernels"] - before)
    pack = pack[args.warmup:]
    hdr = st[:64].cpu().numpy().view(limg_amd.STREAM_HEADER_DTYPE)[0]
    table = st[64:64 + 64 * regions].cpu().numpy().view(limg_amd.STREAM_RECT_DTYPE)
    payload = int(hdr["payloadWords"]) * 8
    # bytes the packer moves: factor bytes of the fields present (payload bits / b * 8 = one byte per value: per rectangle n per field present) + noise of dithered fields + stream
    sh = np.stack([(table["shift"] >> (8 * k)) & 0xFF for k in range(3)], axis=1).astype(np.int64)
    esc = np.stack([(table["shift"] >> (24 + k)) & 1 for k in range(3)], axis=1).astype(np.int64)
    npx = table["rx"].astype(np.int64) * table["ry"] * 64
    present = ((sh < 8) | (esc == 1)).sum(axis=1)
    dithered = ((sh > 0) & (sh < 8)).sum(axis=1)
    pack_bytes = int((npx * (present + dithered)).sum()) + 64 * regions * 2 + 80 * regions + payload
    out["stream_bytes"] = int(nbytes)
    out["rectangles"] = regions
    out["stream_bits_per_pixel"] = round(nbytes * 8.0 / px, 4)
    out["pack_ms"] = stats(pack)
    out["pack_bytes"] = pack_bytes
    out["pack_fraction_of_hbm_peak"] = round(pack_bytes / (stats(pack)["median"] * 1e-3) / HBM_PEAK, 4)
    dec_out = torch.empty((n, n), dtype=torch.int32, device="cuda")
    dec = lambda: g.blocked_decode_stream_device(st, nbytes, n, n, out=dec_out)  # noqa: E731
    timed(dec, args.warmup)
    d = timed(dec, args.reps)
    g.check()
    out["decode_ms"] = stats(d)
    out["decode_bytes"] = int(nbytes) + 4 * px + 8 * (px // 64)
    out["decode_fraction_of_hbm_peak"] = round(out["decode_bytes"] / (stats(d)["median"] * 1e-3) / HBM_PEAK, 4)
    # version 1 on the same image, same box
    st1 = torch.empty(g.stream_bound(n, n), dtype=torch.uint8, device="cuda")
    _, n1 = g.encode_stream_device(img, True, out=st1)
    g.profile_begin()
    for _ in range(args.reps):
        g.encode_stream_device(img, True, out=st1, want_size=False)
    torch.cuda.synchronize()
    prof = g.profile_end()
    d1 = timed(lambda: g.decode_stream_device(st1, n1, n, n, out=dec_out), args.warmup + args.reps)[args.warmup:]
    out["v1_stream_bytes"] = int(n1)
    out["v1_stream_bits_per_pixel"] = round(n1 * 8.0 / px, 4)
    out["v1_profile_ms_rows"] = [[round(float(x), 4) for x in row] for row in prof[-4:].tolist()]
    out["v1_decode_ms"] = stats(d1)
    g.check()
    g.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
