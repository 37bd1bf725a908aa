"""The inputs shared by tests/test_float_edges.py (CPU) and tests/test_gpu_float_edges.py (GPU): 8x8 blocks that reach the edges of the float stage -- the
direction fit's skipped pixels, sign flips decided by the preference bias, exact ties, zero and NaN directions, record fields converted from NaN or from k + 0.5,
factors beyond the clamp, every index of the RSQRTPS table and its smallest arguments.  "Reach" is measured, not argued: the oracle counts the events inside its
own fit and factor functions (oracle/limg_oracle.h, "event sink"), and tests/golden/float_edge_coverage.json records what these inputs reached when
tools/make_float_edge_corpus.py chose them.  tests/golden/float_edge_blocks.npz holds the pixels (`px`: 64 per block, 4 channels; `family`: where a block came
from, an index into the manifest's "families").  Not a test module."""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "float_edge_blocks.npz")
MANIFEST = os.path.join(ROOT, "tests", "golden", "float_edge_coverage.json")
PER_ROW = 64  # blocks per row of the tiled image: 512 pixels wide

LANE_PAIRS = {4: [(a, b) for a in range(4) for b in range(4) if a != b], 3: [(a, b) for a in range(3) for b in range(3) if a != b]}


def required_cells(channels):
    """The cells the corpus must reach on whole blocks (n == 64) with `channels` channels, by their names in oracle.bind.Events (without /context/channels)."""
    req = ["skip.p1", "skip.p2", "flip.p1", "noflip.p1", "bias_decides.p1", "dirA_zero_flat", "dirA_zero_nonflat", "dirB_zero", "dirC_zero", "rec_indefinite",
           "nzA_false", "nzB_false", "nzC_false", "fac_below", "fac_above", "fac_tie"]
    if channels == 4:
        req += ["skip.p3", "dirC_nan", "rec_tie"]
    req += ["tie.p1.%d%d.%s" % (a, b, c) for a, b in LANE_PAIRS[channels] for c in ("lt2", "ge8")]
    return req


# partial blocks (the cropped image) and region fits (the merged-block image) must reach at least these
REQUIRED_ELSEWHERE = ("skip.p1", "dirB_zero", "rec_indefinite", "bias_decides.p1")
# looked for, not required: reported in the manifest as reached or not
ATTEMPTED = {3: ["rec_tie"] + ["tie.p1.%d%d.2to8" % p for p in LANE_PAIRS[3]], 4: ["tie.p1.%d%d.2to8" % p for p in LANE_PAIRS[4]]}


def stored_blocks():
    return np.load(GOLDEN)["px"]


def manifest():
    return json.load(open(MANIFEST))


def tile(px):
    """blocks (N, 64) -> an image of whole blocks, PER_ROW blocks per row; the last row is filled up with the first blocks again"""
    n = len(px)
    rows = (n + PER_ROW - 1) // PER_ROW
    idx = np.arange(rows * PER_ROW) % n
    return np.ascontiguousarray(px[idx].reshape(rows, PER_ROW, 8, 8).transpose(0, 2, 1, 3).reshape(rows * 8, PER_ROW * 8))


def whole_image(px=None):
    return tile(stored_blocks() if px is None else px)


def cropped_image(px=None):
    """the whole-block image without its last 3 columns and 5 rows: the last block column is 5 pixels wide, the last block row 3 high"""
    return np.ascontiguousarray(whole_image(px)[:-5, :-3])


def tiny_images(px=None):
    """1x1, 3x1 and 2x65 (w x h): blocks of fewer than 4 pixels, cut from the corpus -- the 3 x 1 from the first row of the first block whose first three pixels differ,
    the 2 x 65 from the left columns of nine blocks (its last block is 2 x 1)"""
    px = stored_blocks() if px is None else px
    b = next(p for p in px if len({int(p[0]), int(p[1]), int(p[2])}) == 3)
    col = np.concatenate([p.reshape(8, 8)[:, :2] for p in px[:: max(1, len(px) // 9)][:9]])
    return [np.ascontiguousarray(b[:1].reshape(1, 1)), np.ascontiguousarray(b[:3].reshape(1, 3)), np.ascontiguousarray(col[:65])]


def merged_image(px=None):
    """For the merged-block encoder: two block rows of the corpus, then rectangles made to merge -- flat runs of several widths, slow one-channel ramps, a flat field
    with one outlier pixel, and fields of two colours whose channel differences are equal and opposite (every block alike, every pixel on an exact tie)."""
    px = stored_blocks() if px is None else px
    top = tile(px)[:16]
    w = top.shape[1]
    x = np.arange(w, dtype=np.uint32)[None, :]
    y = np.arange(16, dtype=np.uint32)[:, None]
    flat = np.zeros((16, w), dtype=np.uint32)
    for x0, x1, c in ((0, 64, 0xFF336699), (64, 72, 0xFF000000), (72, 200, 0x80FFFFFF), (200, 216, 0x00000000), (216, 512, 0xFF102030)):
        flat[:, x0:x1] = c
    ramp = np.zeros((32, w), dtype=np.uint32)
    ramp[:16] = 0xFF400000 | (x // 4) << 8                      # green rises by 1 every 4 pixels
    ramp[16:] = 0x40000000 | 0x00302010 | ((x // 8) << 24)      # alpha rises by 1 every 8 pixels (3 channels: flat)
    field = np.full((32, w), 0xFF808080, dtype=np.uint32)
    field[13, 77] = 0xFF808180                                  # one pixel, one channel, one step
    field[20, 300] = 0x00FFFFFF
    tie = np.zeros((16, w), dtype=np.uint32)
    odd = ((x[:, :128] + y) & 1).astype(np.uint32)
    tie[:, :128] = 0xFF000000 | (100 + 2 * odd) | ((102 - 2 * odd) << 8) | (50 << 16)           # red / green differ by +-2: ties of magnitude 1
    tie[:, 128:256] = 0xFF000000 | (100 << 0) | ((60 + 10 * odd) << 8) | ((70 - 10 * odd) << 16)  # green / blue by +-10: magnitude 5
    tie[:, 256:384] = (90 << 0) | (90 << 8) | ((40 + 40 * odd) << 16) | ((200 - 40 * odd) << 24)  # blue / alpha by +-40: magnitude 20
    tie[:, 384:] = 0xFF000000 | ((7 + odd) << 0) | (9 << 8) | ((8 - odd) << 16)                  # red / blue by +-1: magnitude 0.5
    return np.ascontiguousarray(np.concatenate([top, flat, ramp, field, tie]).astype(np.uint32))


def degenerate_blocks_image():
    """the hand-made image of tests/test_gpu_parity.py::test_degenerate_blocks: flat blocks, a line, a plane, extreme values, one block row of random bytes"""
    img = np.zeros((16, 256), dtype=np.uint32)
    img[:, :] = 0xFF804020
    x = np.arange(256, dtype=np.uint32)[None, :]
    y = np.arange(16, dtype=np.uint32)[:, None]
    img[0:8, 8:16] = ((10 + 20 * (x[:, 8:16] - 8)) | ((200 - 10 * (x[:, 8:16] - 8)) << 8) | ((50 + 5 * (x[:, 8:16] - 8)) << 16) | (255 << 24))
    img[0:8, 16:24] = ((10 + 20 * (x[:, 16:24] - 16)) | ((30 + 25 * y[0:8]) << 8) | ((50 + 5 * (x[:, 16:24] - 16) + 3 * y[0:8]) << 16) | (255 << 24)).astype(np.uint32)
    img[0:8, 24:32] = 0
    img[0:8, 32:40] = 0xFFFFFFFF
    img[0:8, 40:48] = np.where((x[:, 40:48] + y[0:8]) % 2 == 0, 0, 0xFFFFFFFF).astype(np.uint32)
    rng = np.random.default_rng(3)
    img[8:16, :] = rng.integers(0, 2**32, (8, 256), dtype=np.uint32)
    return img


def events_of(oracle, img, alpha, blocked=False):
    """the oracle's events over one encode of `img` (one worker) -> oracle.bind.Events"""
    with oracle.count_events() as ev:
        if blocked:
            oracle.blocked_encode3d(img, alpha, planes=False)
        else:
            oracle.encode3d(img, alpha, planes=False)
    return ev


def summary(ev, context, channels):
    """what one (context, channels) cell group reached: {"cells": {name: count}, "table_indices": pass-1 indices hit, "min_exponent": ...}"""
    suffix = "/%s/%d" % (context, channels)
    return {"cells": {k[:-len(suffix)]: v for k, v in sorted(ev.cells().items()) if k.endswith(suffix)},
            "table_indices": int(np.count_nonzero(ev.rsq_index(context, channels))), "min_exponent": ev.min_exponent(context, channels)}


def coverage(oracle, px=None):
    """{"whole" | "partial" | "tiny" | "region": {"3" | "4": summary}}: the whole-block image's whole blocks, the cropped image's partial blocks, the tiny shapes'
    blocks of fewer than 4 pixels and the merged image's region fits"""
    out = {}
    for ch in (3, 4):
        alpha = ch == 4
        out.setdefault("whole", {})[str(ch)] = summary(events_of(oracle, whole_image(px), alpha), "whole", ch)
        out.setdefault("partial", {})[str(ch)] = summary(events_of(oracle, cropped_image(px), alpha), "partial", ch)
        with oracle.count_events() as ev:
            for img in tiny_images(px):
                oracle.encode3d(img, alpha, planes=False)
        out.setdefault("tiny", {})[str(ch)] = summary(ev, "tiny", ch)
        out.setdefault("region", {})[str(ch)] = summary(events_of(oracle, merged_image(px), alpha, blocked=True), "region", ch)
    return out
