"""The inputs shared by tests/test_search_hot.py (CPU: they reach every state and edge of the generated hot subtree) and tests/test_gpu_search_hot.py (GPU: the
library encodes them bit for bit like the oracle).  512x64 images -- 512 whole 8x8 blocks, more than one work strip per block row -- of photo-noise, random-gradient
and uniform random bytes, at errorFactor 0 .. 1000, in 3 and 4 channels."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

W, H = 512, 64
ERROR_FACTORS = (0, 10, 25, 50, 100, 200, 400, 1000)
KINDS = ("photo_noise", "random_gradient", "random_bytes")


def image(oracle, kind, w=W, h=H):
    if kind == "photo_noise":
        return oracle.photo_noise(w, h, 7)
    if kind == "random_gradient":
        return oracle.random_gradient(w, h, 7, True)
    return np.random.default_rng(7).integers(0, 2 ** 32, size=(h, w), dtype=np.uint64).astype(np.uint32)


def cases():
    """(kind, has_alpha, errorFactor) of every encode; 4 channels first (tests/test_search_hot.py stops replaying once every edge has been seen)"""
    return [(kind, alpha, ef) for alpha in (True, False) for kind in KINDS for ef in ERROR_FACTORS]


def visited_edges(oracle, img, alpha, ef):
    """{(state path, outcome)} over the whole blocks of `img`: the default search replayed per block with the oracle's trial"""
    from make_search_table import search_fast
    ch = 4 if alpha else 3
    x = oracle.encode3d(img, alpha, planes=False, extras=True, error_factor=ef)
    h, w = img.shape
    seen = set()
    for by in range(h // 8):
        for bx in range(w // 8):
            sl = (slice(by * 8, by * 8 + 8), slice(bx * 8, bx * 8 + 8))
            px = np.ascontiguousarray(img[sl]).ravel()
            rec = np.ascontiguousarray(x["records"][by, bx:bx + 1])
            a, b, c = (np.ascontiguousarray(x[k][sl]).ravel() for k in ("preA", "preB", "preC"))
            g = search_fast()
            path = ""
            try:
                t = next(g)
                while True:
                    ok, _ = oracle.block_trial(px, ch, rec, a, b, c, t, ef)
                    seen.add((path, ok))
                    path += "P" if ok else "F"
                    t = g.send(ok)
            except StopIteration as e:
                assert list(e.value) == x["shifts"][by, bx].tolist(), (by, bx, e.value)
    return seen


def rare_edge_images():
    """Blocks that take the hot subtree's rare edges (a coarser trial passing after finer ones failed: a few blocks in a million of natural content), found by a
    CPU search over synthetic blocks with the oracle's trial and kept in tests/golden/search_hot_blocks.npz (`px`: 64 pixels per block, `ef`: the errorFactor at
    which the block takes its edge).  One image of whole blocks, 8 pixels high, per errorFactor -> [(image, errorFactor)]."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "search_hot_blocks.npz"))
    out = []
    for ef in sorted(set(z["ef"].tolist())):
        blocks = z["px"][z["ef"] == ef]
        out.append((np.ascontiguousarray(np.concatenate([b.reshape(8, 8) for b in blocks], axis=1)), int(ef)))
    return out


def coverage_inputs(oracle):
    """[(image, has_alpha, errorFactor)]: the rare-edge images first, then every generated image of cases()"""
    out = [(img, True, ef) for img, ef in rare_edge_images()]
    imgs = {kind: image(oracle, kind) for kind in KINDS}
    return out + [(imgs[kind], alpha, ef) for kind, alpha, ef in cases()]
