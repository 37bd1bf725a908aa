"""The inputs shared by tests/test_block_verdict.py (CPU) and tests/test_gpu_block_verdict.py (GPU): whole 8x8 blocks on the edge of the block-sum verdict of the
default shift search.  A trial passes when no pixel is over its limit and the block's error sum is BELOW blockLimit (be * 16 < maxBlock * 64, i.e.
be < 112 * (errorFactor / 2) for a whole block); the kernels decide that on one lane's compare, so the blocks kept here have a trial -- one the default search
really runs on them -- whose sum is exactly blockLimit - 1 (must pass) or exactly blockLimit (must fail).

tests/golden/block_verdict_blocks.npz holds them: `px` (64 pixels per block, 4 channels), `ef` (the errorFactor at which the block has its edge trial) and `kind`
(0: a sum of blockLimit - 1, 1: a sum of blockLimit).  They come from photo-noise images; run this file to scan again:  python tests/block_verdict_inputs.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

GOLDEN = os.path.join(ROOT, "tests", "golden", "block_verdict_blocks.npz")
BELOW, AT = 0, 1  # kinds: the sum is blockLimit - 1 / the sum is blockLimit


def block_limit(ef):
    """blockLimit of a whole block: the smallest sum that fails (maxBlock = 4 * (ef / 2) * 7, be * 16 < maxBlock * 64)"""
    return 4 * (ef // 2) * 7 * 64 // 16


def edge_trials(oracle, img, ef, alpha=True):
    """{(by, bx): set of kinds} over the whole blocks of `img`: the default search replayed per block with the oracle's trial; a kind is recorded where a trial
    without a failing pixel (a failing pixel reports no sum) has a block sum of exactly blockLimit - 1 (and passes) or blockLimit (and fails)"""
    from make_search_table import search_fast
    ch = 4 if alpha else 3
    x = oracle.encode3d(img, alpha, planes=False, extras=True, error_factor=ef)
    h, w = img.shape
    lim = block_limit(ef)
    found = {}
    for by in range(h // 8):
        for bx in range(w // 8):
            sl = (slice(by * 8, by * 8 + 8), slice(bx * 8, bx * 8 + 8))
            px = np.ascontiguousarray(img[sl]).ravel()
            rec = np.ascontiguousarray(x["records"][by, bx:bx + 1])
            a, b, c = (np.ascontiguousarray(x[k][sl]).ravel() for k in ("preA", "preB", "preC"))
            g = search_fast()
            try:
                t = next(g)
                while True:
                    ok, be = oracle.block_trial(px, ch, rec, a, b, c, t, ef)
                    if ok and be == lim - 1:
                        found.setdefault((by, bx), set()).add(BELOW)
                    if not ok and be == lim:
                        found.setdefault((by, bx), set()).add(AT)
                    assert ok == (be < lim) or (not ok and be == 0), (by, bx, t, ok, be)
                    t = g.send(ok)
            except StopIteration as e:
                assert list(e.value) == x["shifts"][by, bx].tolist(), (by, bx, e.value)
    return found


def stored_blocks():
    z = np.load(GOLDEN)
    return z["px"], z["ef"], z["kind"]


def edge_images():
    """the stored blocks tiled into one image of whole blocks, 8 pixels high, per errorFactor -> [(image, errorFactor, kinds in block order)]"""
    px, efs, kinds = stored_blocks()
    out = []
    for ef in sorted(set(efs.tolist())):
        sel = efs == ef
        out.append((np.ascontiguousarray(np.concatenate([b.reshape(8, 8) for b in px[sel]], axis=1)), int(ef), kinds[sel].tolist()))
    return out


def scan(oracle, error_factors=(25, 50, 100), seeds=range(1, 25), per_kind=6, w=512, h=64):
    """photo-noise images, seed by seed, until every errorFactor has `per_kind` blocks of each kind (or the seeds run out)"""
    px, efs, kinds = [], [], []
    for ef in error_factors:
        have = {BELOW: 0, AT: 0}
        for seed in seeds:
            if min(have.values()) >= per_kind:
                break
            img = oracle.photo_noise(w, h, seed)
            for (by, bx), ks in sorted(edge_trials(oracle, img, ef).items()):
                for k in sorted(ks):
                    if have[k] < per_kind:
                        have[k] += 1
                        px.append(np.ascontiguousarray(img[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8]).ravel())
                        efs.append(ef)
                        kinds.append(k)
        print("errorFactor %d: %d blocks at limit - 1, %d at limit" % (ef, have[BELOW], have[AT]), flush=True)
    return np.array(px, dtype=np.uint32), np.array(efs, dtype=np.uint32), np.array(kinds, dtype=np.uint8)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    from oracle.bind import Oracle
    px, efs, kinds = scan(Oracle())
    np.savez_compressed(GOLDEN, px=px, ef=efs, kind=kinds)
    print("wrote", GOLDEN, len(px), "blocks")
