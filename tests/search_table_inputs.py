"""The inputs shared by tests/test_search_tables.py (CPU: replayed with the oracle's trial they reach every class of edges of the accurate search's automaton and of
the default table outside its hot subtree) and tests/test_gpu_search_tables.py (GPU: the library encodes them bit for bit like the oracle).  The images and rare-edge
blocks of tests/search_hot_inputs.py, 512x16 images of the same three generators at low and very high errorFactors, and the blocks of
tests/golden/search_table_blocks.npz (found by tools/search_table_blocks.py), all of whole 8x8 blocks."""
import os

import numpy as np

import search_hot_inputs as hot  # (puts tools/ on sys.path)

ROOT = hot.ROOT
LOW_W, LOW_H = 512, 16
ACCURATE_LOW_EF = (5,)  # the only 4-channel inputs on which A and B change and C stays after a passing phase-2 trial (in 3 channels random bytes do it too)
DEFAULT_LOW_EF = (0, 5, 2000, 3000)
PARTIAL_W, PARTIAL_H = 508, 61
PARTIAL_EF = (5, 25, 100, 1000)
BLOCKED_EF = (5, 25, 100, 400)
GOLDEN_BLOCKS = os.path.join(ROOT, "tests", "golden", "search_table_blocks.npz")


def _name(what, img, alpha, ef):
    return "%s %dx%d, %d channels, errorFactor %d" % (what, img.shape[1], img.shape[0], 4 if alpha else 3, ef)


def low_images(oracle):
    return {kind: hot.image(oracle, kind, LOW_W, LOW_H) for kind in hot.KINDS}


def _hot_corpus(oracle, strip_alphas=(True,)):
    out = [(_name("rare-edge strip", img, alpha, ef), img, alpha, ef) for alpha in strip_alphas for img, ef in hot.rare_edge_images()]
    imgs = {kind: hot.image(oracle, kind) for kind in hot.KINDS}
    return out + [(_name(kind, imgs[kind], alpha, ef), imgs[kind], alpha, ef) for kind, alpha, ef in hot.cases()]


def found_block_images():
    """Blocks that take edges of the default table which the generated images do not (tools/search_table_blocks.py; `px`: 64 pixels per block, `ef`: the errorFactor
    at which a block takes its edge, `alpha`: 1 where it does so in 4 channels).  One image of whole blocks, 8 pixels high, per (errorFactor, channels)
    -> [(image, has_alpha, errorFactor)]; none if the search found nothing to keep."""
    if not os.path.exists(GOLDEN_BLOCKS):
        return []
    z = np.load(GOLDEN_BLOCKS)
    out = []
    for ef, alpha in sorted(set(zip(z["ef"].tolist(), z["alpha"].tolist()))):
        blocks = z["px"][(z["ef"] == ef) & (z["alpha"] == alpha)]
        out.append((np.ascontiguousarray(np.concatenate([b.reshape(8, 8) for b in blocks], axis=1)), bool(alpha), int(ef)))
    return out


def accurate_inputs(oracle):
    """[(name, image, has_alpha, errorFactor)] of the accurate search: the rare-edge strips first (in 3 channels too: one of them is the only 3-channel input that
    rebuilds C alone after a failing phase-1 trial), then 4 channels before 3"""
    low = low_images(oracle)
    return _hot_corpus(oracle, (True, False)) + [(_name(kind, low[kind], alpha, ef), low[kind], alpha, ef) for alpha in (True, False) for kind in hot.KINDS for ef in ACCURATE_LOW_EF]


def default_inputs(oracle):
    """[(name, image, has_alpha, errorFactor)] of the default search"""
    low = low_images(oracle)
    out = [(_name("found-block strip", img, alpha, ef), img, alpha, ef) for img, alpha, ef in found_block_images()] + _hot_corpus(oracle)
    return out + [(_name(kind, low[kind], alpha, ef), low[kind], alpha, ef) for alpha in (True, False) for kind in hot.KINDS for ef in DEFAULT_LOW_EF]


def partial_inputs(oracle):
    """[(name, image, errorFactor)]: crops with partial blocks at the right and bottom edges (the kernels' FULL == false walk, from the root of either table)"""
    crops = {kind: np.ascontiguousarray(hot.image(oracle, kind)[:PARTIAL_H, :PARTIAL_W]) for kind in hot.KINDS}
    return [("%s crop %dx%d, errorFactor %d" % (kind, PARTIAL_W, PARTIAL_H, ef), crops[kind], ef) for kind in hot.KINDS for ef in PARTIAL_EF]


def blocked_inputs(oracle):
    """[(name, image, has_alpha, errorFactor)] of the merged-block encoder's accurate search (the literal loops): every rare-edge strip and the 512x16 images at
    each errorFactor of BLOCKED_EF"""
    low = low_images(oracle)
    return [(_name("rare-edge strip %d" % i, img, True, ef), img, True, ef) for i, (img, _) in enumerate(hot.rare_edge_images()) for ef in BLOCKED_EF] + \
           [(_name(kind, low[kind], alpha, ef), low[kind], alpha, ef) for alpha in (True, False) for kind in hot.KINDS for ef in BLOCKED_EF]


def blocks_of(oracle, img, alpha, ef, fast):
    """per whole block of `img`: (memoised outcome(a, b, c) -> (passed, block error) of the oracle's trial, the oracle's shifts)"""
    ch = 4 if alpha else 3
    x = oracle.encode3d(img, alpha, planes=False, extras=True, error_factor=ef, fast=fast)
    h, w = img.shape
    for by in range(h // 8):
        for bx in range(w // 8):
            sl = (slice(by * 8, by * 8 + 8), slice(bx * 8, bx * 8 + 8))
            px = np.ascontiguousarray(img[sl]).ravel()
            rec = np.ascontiguousarray(x["records"][by, bx:bx + 1])
            a, b, c = (np.ascontiguousarray(x[k][sl]).ravel() for k in ("preA", "preB", "preC"))
            memo = {}

            def outcome(sa, sb, sc, px=px, rec=rec, a=a, b=b, c=c, memo=memo):
                if (sa, sb, sc) not in memo:
                    memo[(sa, sb, sc)] = oracle.block_trial(px, ch, rec, a, b, c, (sa, sb, sc), ef)
                return memo[(sa, sb, sc)]
            yield outcome, tuple(x["shifts"][by, bx].tolist())
