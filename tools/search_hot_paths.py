#!/usr/bin/env python3
"""The hot part of the default shift search's decision tree -> tools/search_hot_paths.json, the input of tools/make_search_table.py's straight-line code
(limg_amd/csrc/limg_search_hot.h).

A state is the path of outcomes from the root ("" = the first trial, "PF" = after a pass and a fail).  Visits per state are counted over 1500 random 8x8 blocks each of
1024x1024 photo-noise at errorFactor 25 / 50 / 100 / 200 / 400 and random-gradient at 25 / 100 / 400 (RGBA, generator seed 1, block picks from default_rng(11)); the
hot set is every state visited at least 0.25 times per block in ANY of these settings.  Visit counts fall along a path, so the set is closed under prefixes.  The
rule is fixed so that the set is a property of the search and not tuned to one workload.
CPU only (the oracle's trial as the outcome function of the literal restatement of the reference's search); test infrastructure like tools/search_stats.py.
usage: python tools/search_hot_paths.py [--blocks 1500] [--out tools/search_hot_paths.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_search_table import search_fast  # noqa: E402

SETTINGS = [("photo_noise", 25), ("photo_noise", 50), ("photo_noise", 100), ("photo_noise", 200), ("photo_noise", 400),
            ("random_gradient", 25), ("random_gradient", 100), ("random_gradient", 400)]
THRESHOLD = 0.25
SIZE = 1024


def block_paths(orc, px, channels, ef, rec=None, fac=None):
    """the states one block visits, root first, and the shifts its search ends with"""
    if rec is None:
        rec = orc.block_fit(px, channels)
    a, b, c = fac if fac is not None else orc.block_factors(px, channels, rec)
    g = search_fast()
    path = ""
    out = []
    try:
        t = next(g)
        while True:
            out.append(path)
            ok, _ = orc.block_trial(px, channels, rec, a, b, c, t, ef)
            path += "P" if ok else "F"
            t = g.send(ok)
    except StopIteration as e:
        return out, e.value


def main():
    from oracle.bind import Oracle
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=1500)
    ap.add_argument("--out", default=os.path.join(ROOT, "tools", "search_hot_paths.json"))
    args = ap.parse_args()
    orc = Oracle()
    imgs = {"photo_noise": orc.photo_noise(SIZE, SIZE, 1), "random_gradient": orc.random_gradient(SIZE, SIZE, 1, True)}
    rng = np.random.default_rng(11)
    picks = [(int(rng.integers(0, SIZE // 8)), int(rng.integers(0, SIZE // 8))) for _ in range(args.blocks)]
    prepared = {}
    for kind, img in imgs.items():
        prepared[kind] = []
        for bx, by in picks:
            px = np.ascontiguousarray(img[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8]).ravel()
            rec = orc.block_fit(px, 4)
            prepared[kind].append((px, rec, orc.block_factors(px, 4, rec)))
    visits = {}
    names = []
    for kind, ef in SETTINGS:
        name = "%s_ef%d" % (kind, ef)
        names.append(name)
        for px, rec, fac in prepared[kind]:
            for p in block_paths(orc, px, 4, ef, rec, fac)[0]:
                visits.setdefault(p, {}).setdefault(name, 0)
                visits[p][name] += 1
    hot = {p: {n: round(v.get(n, 0) / args.blocks, 4) for n in names} for p, v in visits.items() if max(v.values()) >= THRESHOLD * args.blocks}
    assert all(p[:-1] in hot for p in hot if p), "visit counts fall along a path"
    doc = {"rule": "states (paths of P / F outcomes from the root) with at least %.2f visits per block in any setting" % THRESHOLD,
           "sample": "%d blocks per setting of %dx%d RGBA images, generator seed 1, picks from default_rng(11)" % (args.blocks, SIZE, SIZE),
           "settings": names,
           "states": {p: hot[p] for p in sorted(hot, key=lambda s: (len(s), s))}}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out, len(hot), "states, deepest", max(len(p) for p in hot))


if __name__ == "__main__":
    main()
