#!/usr/bin/env python3
"""Search synthetic 8x8 blocks that take given edges of the default shift search's decision table (limg_search_table.h) -- the edges of the classes that the
generated images of tests/search_table_inputs.py do not reach -- and keep them in tests/golden/search_table_blocks.npz.

An edge is named by the path of pass / fail outcomes that leads to it.  A trial of a triple passes at errorFactor 2 h iff every pixel error is <= 42 h and their
sum is < 112 h (the oracle's thresholds), so a block has, per triple, a smallest h from which on the triple passes; the block takes the edge at some errorFactor
iff the largest such h over the triples that must pass lies below the smallest over the triples that must fail.  That difference is the objective of a hill climb
over single-pixel changes, restarted from random blocks spread along three colour directions (uniform, two-valued and clustered factor distributions).

    python tools/search_table_blocks.py [--seconds N] [--workers N]      (CPU only: the oracle's fit, factors and per-pixel trial errors)
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_search_table as mst  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "search_table_blocks.npz")
CLASSES = {"rebuild B+C after a pass": (6, True), "rebuild A+B+C after a pass": (7, True)}  # (change mask of the successor, outcome) of edges that leave non-hot states


def targets():
    """[(class name, path to the edge incl. its own outcome, {triple: must pass})] for every edge of CLASSES that leaves a non-hot state"""
    trans = mst.build()
    words = mst.encode(trans)
    hot = {n["sid"] for n in mst.hot_nodes(mst.hot_tree(trans, mst.load_hot_paths()))}
    out = []

    def visit(s, path, need):
        t = trans[s]
        if t[0] == "final":
            return
        for ok in (True, False):
            n = t[1 if ok else 2]
            need2 = dict(need)
            need2[tuple(t[0])] = ok
            if s not in hot and trans[n][0] != "final":
                for name, (mask, outcome) in CLASSES.items():
                    if ok == outcome and (words[n][0] >> 5) & 7 == mask:
                        out.append((name, path + ("P" if ok else "F"), need2))
            visit(n, path + ("P" if ok else "F"), need2)

    visit(0, "", {})
    return out


class Trial:
    def __init__(self):
        from oracle.bind import Oracle
        self.o = Oracle()
        self.f = self.o.lib.limg_oracle_block_trial_pixel_errors
        self.f.restype = None
        self.f.argtypes = [C.c_void_p, C.c_size_t, C.c_int] + [C.c_void_p] * 6
        self.err = np.zeros(64, dtype=np.uint32)

    def first_h(self, px, channels, triples):
        """{triple: the smallest h = errorFactor // 2 at which its trial passes}"""
        rec = self.o.block_fit(px, channels)
        a, b, c = self.o.block_factors(px, channels, rec)
        out = {}
        for t in triples:
            sh = np.asarray(t, dtype=np.uint8)
            self.f(px.ctypes.data, 64, channels, rec.ctypes.data, a.ctypes.data, b.ctypes.data, c.ctypes.data, sh.ctypes.data, self.err.ctypes.data)
            out[t] = max((int(self.err.max()) + 41) // 42, int(self.err.sum(dtype=np.uint64)) // 112 + 1)
        return out


def margin(tr, px, channels, need):
    h = tr.first_h(px, channels, list(need))
    lo = max(h[t] for t, ok in need.items() if ok)
    hi = min(h[t] for t, ok in need.items() if not ok)
    return hi - lo, lo


def random_block(rng):
    base = rng.integers(40, 216, 3).astype(np.float64)
    dirs = rng.normal(size=(3, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    amp = np.array([rng.uniform(20, 160), rng.uniform(4, 80), rng.uniform(1, 40)])
    f = np.empty((3, 64))
    for k in range(3):
        kind = rng.integers(0, 3)
        if kind == 0:
            f[k] = rng.uniform(-1, 1, 64)
        elif kind == 1:
            f[k] = rng.choice((-1.0, 1.0), 64) * rng.uniform(0.7, 1.0, 64)
        else:
            f[k] = rng.choice(rng.uniform(-1, 1, 4), 64) + rng.normal(0, 0.05, 64)
    col = base[None, :] + (f * amp[:, None]).T @ dirs + rng.normal(0, rng.uniform(0, 2), (64, 3))
    col = np.clip(np.rint(col), 0, 255).astype(np.uint32)
    return (col[:, 0] | (col[:, 1] << 8) | (col[:, 2] << 16) | np.uint32(0xFF000000)).astype(np.uint32)


def climb(args):
    """one worker: restarts of the hill climb for one target until `seconds` are over -> (pixels, errorFactor) or None"""
    need, seed, seconds, channels = args
    tr = Trial()
    rng = np.random.default_rng(seed)
    end = time.time() + seconds
    while time.time() < end:
        px = random_block(rng)
        m, lo = margin(tr, px, channels, need)
        stale = 0
        while m < 1 and stale < 300 and time.time() < end:
            q = px.copy()
            for _ in range(int(rng.integers(1, 4))):
                i, c = int(rng.integers(0, 64)), int(rng.integers(0, 3))
                v = int((q[i] >> (8 * c)) & 0xFF) + int(rng.integers(-6, 7))
                q[i] = (int(q[i]) & ~(0xFF << (8 * c))) | (min(255, max(0, v)) << (8 * c))
            m2, lo2 = margin(tr, q, channels, need)
            if m2 >= m:
                stale = 0 if m2 > m else stale + 1
                px, m, lo = q, m2, lo2
            else:
                stale += 1
        if m >= 1:
            return px, 2 * lo
    return None


def main():
    import multiprocessing as mp
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=120)
    ap.add_argument("--workers", type=int, default=8)
    a = ap.parse_args()
    found = []
    with mp.Pool(a.workers) as pool:
        for name, path, need in targets():
            for channels in (4, 3):
                got = [r for r in pool.map(climb, [(need, 1000 * channels + w, a.seconds, channels) for w in range(a.workers)]) if r is not None]
                print("%s, path %s, %d channels: %d of %d workers found a block" % (name, path, channels, len(got), a.workers), flush=True)
                if got:
                    found.append((got[0][0], got[0][1], channels == 4, "%s: %s" % (name, path)))
    if found:
        np.savez(OUT, px=np.array([f[0] for f in found], dtype=np.uint32), ef=np.array([f[1] for f in found], dtype=np.uint32),
                 alpha=np.array([f[2] for f in found], dtype=np.uint8), edge=np.array([f[3] for f in found]))
        print("wrote", OUT, len(found), "blocks")


if __name__ == "__main__":
    main()
