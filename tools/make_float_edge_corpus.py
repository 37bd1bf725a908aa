#!/usr/bin/env python3
"""Builds tests/golden/float_edge_blocks.npz and tests/golden/float_edge_coverage.json (see tests/float_edge_inputs.py).  CPU only.

Seeded families of 8x8 blocks go, block by block, through the oracle's fit and factor functions with its event sink on, with 3 and with 4 channels.  A block
is kept when it adds an (event, context, channels) cell or a pass-1 RSQRTPS table index that no kept block has reached; the first few blocks of every family and
the blocks with the smallest RSQRTPS arguments are kept besides.  The kept pixels are stored, and the coverage measured on the images of tests/float_edge_inputs.py is written next to them.

Families:
  flat            one colour
  two_colour      k of 64 pixels in a second colour; differences of one step in one channel up to the full range
  opposite        two colours whose differences in two channels are equal and opposite, as a checkerboard and as a random 32 / 32 split: every pixel on an exact
                  tie -min == max.  Every lane pair, half differences below 2 (0.5, 1, 1.5), from 2 to below 8, and 8 and up.  Odd differences put the average on
                  k + 0.5 (the 3-channel record tie; the checkerboard of a large difference has dirA == 0, so its record is the average)
  ramp / noise1   one channel ramps or carries noise, the others stand still (dirB == 0, NaN extrema)
  noise           amplitude 1..3 around a base colour
  line / plane    points on a line / in a plane of colour space
  low             colours of a few steps around 0 and 255 (small averages: the smallest residues of pass 2 and 3)
  index           pixel pairs base +- v with integer v: the RSQRTPS argument is the integer |v|^2, chosen per table index (odd exponent: 4096..8191, even: 8192..16383)
  bytes           random bytes
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import float_edge_inputs as F  # noqa: E402
from oracle.bind import Oracle  # noqa: E402

FAMILIES = ("flat", "two_colour", "opposite", "ramp", "noise1", "noise", "line", "plane", "low", "index", "bytes")
FAMILY_KEPT = 6  # blocks of every family kept whatever they add
LOWEST_KEPT = 8  # blocks kept for the smallest RSQRTPS exponents, per channel count


def pack(c):
    """(..., 4) channel values -> pixels"""
    c = np.clip(np.asarray(c), 0, 255).astype(np.uint32)
    return c[..., 0] | (c[..., 1] << 8) | (c[..., 2] << 16) | (c[..., 3] << 24)


def flat(rng):
    return np.full(64, pack(rng.integers(0, 256, 4)), dtype=np.uint32)


def two_colour(rng):
    c0 = rng.integers(0, 256, 4)
    kind = rng.integers(0, 3)
    d = np.zeros(4, dtype=np.int64)
    if kind == 0:
        d[rng.integers(0, 4)] = rng.choice([-2, -1, 1, 2])
    elif kind == 1:
        d = rng.integers(-3, 4, 4)
    else:
        d = rng.integers(-255, 256, 4) * (rng.random(4) < 0.6)
    c1 = np.clip(c0 + d, 0, 255)
    k = int(rng.choice([1, 2, 3, 31, 32, 33, 61, 62, 63, rng.integers(1, 64)]))
    sel = np.zeros(64, dtype=bool)
    sel[rng.permutation(64)[:k] if rng.random() < 0.5 else np.arange(k)] = True
    return np.where(sel, pack(c1), pack(c0)).astype(np.uint32)


def opposite(rng, a=None, b=None, diff=None, checker=None):
    a, b = (rng.permutation(4)[:2] if a is None else (a, b))
    diff = int(rng.choice([1, 2, 3, 4, 5, 7, 10, 14, 15, 16, 17, 31, 64, 101, 255])) if diff is None else diff
    c0 = rng.integers(0, 256 - diff, 4)
    c1 = c0.copy()
    c1[a] += diff
    c0[b] += diff
    if checker is None:
        checker = rng.random() < 0.5
    sel = ((np.arange(64) // 8 + np.arange(64)) & 1).astype(bool) if checker else np.isin(np.arange(64), rng.permutation(64)[:32])
    return np.where(sel, pack(c1), pack(c0)).astype(np.uint32)


def ramp(rng):
    c = np.tile(rng.integers(0, 200, 4), (64, 1))
    x, y = np.arange(64) % 8, np.arange(64) // 8
    t = [x, y, x + y, x * 8 + y][rng.integers(0, 4)]
    c[:, rng.integers(0, 4)] = rng.integers(0, 60) + t * rng.integers(1, 4)
    return pack(c)


def noise1(rng):
    c = np.tile(rng.integers(0, 256, 4), (64, 1))
    c[:, rng.integers(0, 4)] = rng.integers(0, 256, 64) if rng.random() < 0.5 else rng.integers(0, 256) + rng.integers(-2, 3, 64)
    return pack(c)


def noise(rng):
    amp = rng.integers(1, 4)
    return pack(rng.integers(0, 256, 4)[None, :] + rng.integers(-amp, amp + 1, (64, 4)))


def line(rng):
    t = rng.integers(-8, 9, 64)[:, None]
    return pack(rng.integers(60, 190, 4)[None, :] + t * rng.integers(-6, 7, 4)[None, :])


def plane(rng):
    t, u = rng.integers(-6, 7, 64)[:, None], rng.integers(-6, 7, 64)[:, None]
    return pack(rng.integers(80, 170, 4)[None, :] + t * rng.integers(-5, 6, 4)[None, :] + u * rng.integers(-5, 6, 4)[None, :])


def low(rng):
    base = np.where(rng.random(4) < 0.5, 0, 255) if rng.random() < 0.5 else np.zeros(4, dtype=np.int64)
    span = rng.integers(1, 4)
    c = np.abs(base[None, :] - rng.integers(0, span + 1, (64, 4)) * (rng.random((64, 1)) < rng.choice([0.05, 0.3, 0.7])))
    return pack(c)


def _squares(target, lanes):
    """integers v (|v| <= 127, `lanes` of them) with sum v^2 == target, or None"""
    best = None
    r = int(target ** 0.5)
    for a in range(min(r, 127), -1, -1):
        ra = target - a * a
        for b in range(min(int(ra ** 0.5), a), -1, -1):
            rb = ra - b * b
            c = int(rb ** 0.5 + 0.5)
            if lanes >= 3 and c * c == rb and c <= 127:
                return [a, b, c]
            if lanes == 2 and rb == 0:
                return [a, b]
    return best


def index_blocks(rng):
    """every table index once, 32 per block: the vector's alpha lane is 0, so 3 and 4 channels see the same argument"""
    vecs = []
    for parity_base, lo, per in ((0, 4096, 4), (1024, 8192, 8)):  # biased exponent 139 (odd: indices 0..1023), 140 (even: 1024..2047)
        for m in range(1024):
            v = None
            for t in range(lo + m * per, lo + (m + 1) * per):
                v = _squares(t, 3)
                if v:
                    break
            assert v, (parity_base, m)
            vecs.append(v)
    vecs = [vecs[i] for i in rng.permutation(len(vecs))]
    for i in range(0, len(vecs), 32):
        c = np.full((64, 4), 128, dtype=np.int64)
        c[:, 3] = rng.integers(0, 256)
        for k, v in enumerate(vecs[i:i + 32]):
            v = np.array(v)[rng.permutation(3)] * rng.choice([-1, 1], 3)
            c[2 * k, :3] += v
            c[2 * k + 1, :3] -= v
        yield pack(c[rng.permutation(64)])


def rand_bytes(rng):
    return rng.integers(0, 2 ** 32, 64, dtype=np.uint32)


def candidates():
    """(family, pixels) in a fixed order: the designed blocks first, then the seeded draws"""
    rng = np.random.default_rng(20240611)
    for _ in range(4):
        yield "flat", flat(rng)
    for a in range(4):
        for b in range(4):
            if a != b and a < b:
                for diff in (1, 2, 3, 5, 6, 9, 10, 13, 15, 16, 17, 40, 255):
                    for checker in (True, False):
                        yield "opposite", opposite(rng, a, b, diff, checker)
    for blk in index_blocks(rng):
        yield "index", blk
    gens = {"two_colour": (two_colour, 600), "opposite": (opposite, 200), "ramp": (ramp, 150), "noise1": (noise1, 150), "noise": (noise, 300), "line": (line, 200),
            "plane": (plane, 200), "low": (low, 400), "bytes": (rand_bytes, 120), "flat": (flat, 4)}
    for name, (fn, count) in gens.items():
        for _ in range(count):
            yield name, fn(rng)


def block_events(oracle, ev, px):
    """the counters one block moves, 3 and 4 channels: (indices of the scalar cells and pass-1 table indices, smallest exponent)"""
    ev.counters[:] = 0
    for ch in (3, 4):
        rec = oracle.block_fit(px, ch)
        oracle.block_factors(px, ch, rec)
    hit = np.flatnonzero(ev.counters)
    cell = hit % ev.CELL
    keep = (cell < ev.RSQ_INDEX + 2048) | (cell >= ev.FIT)  # passes 2 and 3 of the table and the exponents do not steer the choice
    lo = tuple(255 if e is None else e for e in (ev.min_exponent("whole", 3), ev.min_exponent("whole", 4)))
    return set(hit[keep].tolist()), lo


def main():
    oracle = Oracle()
    kept, fams, covered, lows, seen = [], [], set(), [], 0
    with oracle.count_events() as ev:
        for fam, px in candidates():
            seen += 1
            hit, lo = block_events(oracle, ev, px)
            if hit - covered or fams.count(FAMILIES.index(fam)) < FAMILY_KEPT:
                covered |= hit
                kept.append(px)
                fams.append(FAMILIES.index(fam))
            lows.append((lo, seen, fam, px))
    have = {p.tobytes() for p in kept}
    for ch in (0, 1):  # the smallest arguments with 3 and with 4 channels, whether or not the block was kept for a cell
        for lo, _, fam, px in sorted(lows, key=lambda t: (t[0][ch], t[1]))[:LOWEST_KEPT]:
            if px.tobytes() not in have:
                have.add(px.tobytes())
                kept.append(px)
                fams.append(FAMILIES.index(fam))
    px = np.array(kept, dtype=np.uint32)
    fams = np.array(fams, dtype=np.uint8)
    print("%d candidates, %d blocks kept: %s" % (seen, len(px), {f: int((fams == i).sum()) for i, f in enumerate(FAMILIES)}))

    cov = F.coverage(oracle, px)
    missing = {ch: [c for c in F.required_cells(ch) if c not in cov["whole"][str(ch)]["cells"]] for ch in (3, 4)}
    missing.update({"%s/%d" % (ctx, ch): [c for c in F.REQUIRED_ELSEWHERE if c not in cov[ctx][str(ch)]["cells"]] for ctx in ("partial", "region") for ch in (3, 4)})
    man = {"blocks": len(px), "families": list(FAMILIES), "blocks_per_family": {f: int((fams == i).sum()) for i, f in enumerate(FAMILIES)}, "coverage": cov,
           "required_missing": {str(k): v for k, v in missing.items() if v},
           "attempted": {str(ch): {c: c in cov["whole"][str(ch)]["cells"] for c in F.ATTEMPTED[ch]} for ch in (3, 4)}}
    for ctx in cov:
        for ch in cov[ctx]:
            print(ctx, ch, "cells", len(cov[ctx][ch]["cells"]), "table indices", cov[ctx][ch]["table_indices"], "min exponent", cov[ctx][ch]["min_exponent"])
    print("required cells missing:", man["required_missing"] or "none")
    print("attempted:", man["attempted"])
    np.savez_compressed(F.GOLDEN, px=px, family=fams)
    with open(F.MANIFEST, "w") as f:
        json.dump(man, f, indent=1, sort_keys=True)
        f.write("\n")
    ok = not man["required_missing"] and all(cov["whole"][ch]["table_indices"] == 2048 for ch in ("3", "4"))
    print("wrote", F.GOLDEN, os.path.getsize(F.GOLDEN), "bytes;", "complete" if ok else "INCOMPLETE")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
