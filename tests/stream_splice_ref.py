"""Restatement of the stream splice (include/limg_hip.h "stream splice") in numpy on top of oracle.stream.parse / assemble -- test infrastructure, no GPU.

A piece is (src_w, src_h, src_bx, src_by, dst_bx, dst_by, blocks_w, blocks_h): a rectangle of 8x8 blocks of a source image of src_w x src_h pixels and the place of
its first block in the output's block grid.  The rules are restated block by block, on purpose another way than limg_amd/csrc/limg_hip_splice_plan.h decides them
(which sorts runs and never looks at a block):
  exact cover   every block of the output's grid is claimed by exactly one piece (a counter per block);
  inside        every block of a piece exists in its source's grid;
  edge rule     an output block and the source block it comes from hold the same number of pixel columns and rows (8, or what the image's size leaves of the last
                one): a clipped block only ever comes from a block clipped alike, a whole block from a whole one.
splice_bytes() then builds the expected stream block by block in the output's raster order: the source's entry with payloadWord = the words written so far, and the
source block's words behind them."""
import numpy as np

from oracle import stream as S

ITEM_BLOCKS = 64  # limg_hip_splice_plan.h kSpliceItemBlocks


def blocks(size):
    return (size + 7) // 8


def extent(size, b):
    """pixel columns (rows) of block column (row) b of an image `size` pixels wide (high)"""
    return min(8, size - 8 * b)


def accepted(pieces, w, h):
    if not pieces or w <= 0 or h <= 0:
        return False
    bx, by = blocks(w), blocks(h)
    claimed = np.zeros((by, bx), dtype=np.int64)
    for sw, sh, sbx, sby, dbx, dby, bw, bh in pieces:
        if bw <= 0 or bh <= 0 or sw <= 0 or sh <= 0:
            return False
        if sbx + bw > blocks(sw) or sby + bh > blocks(sh) or dbx + bw > bx or dby + bh > by:
            return False
        if any(extent(w, dbx + i) != extent(sw, sbx + i) for i in range(bw)) or any(extent(h, dby + j) != extent(sh, sby + j) for j in range(bh)):
            return False
        claimed[dby:dby + bh, dbx:dbx + bw] += 1
    return bool((claimed == 1).all())


def runs(pieces, w, h):
    """the run list of an accepted call: (piece, srcEntry, dstEntry, count) per block row of each piece, in the output's raster order; None where the call is refused"""
    if not accepted(pieces, w, h):
        return None
    bx = blocks(w)
    out = []
    for k, (sw, sh, sbx, sby, dbx, dby, bw, bh) in enumerate(pieces):
        for j in range(bh):
            out.append((k, (sby + j) * blocks(sw) + sbx, (dby + j) * bx + dbx, bw))
    return sorted(out, key=lambda r: r[2])


def items(run_list):
    """the copy kernel's item prefix: one item per ITEM_BLOCKS blocks of a run"""
    base = [0]
    for _, _, _, count in run_list:
        base.append(base[-1] + -(-count // ITEM_BLOCKS))
    return base


def entry_words(e):
    sw = int(e["shift"])
    return sum(8 if (sw >> (24 + k)) & 1 else max(0, 8 - ((sw >> (8 * k)) & 0xFF)) for k in range(3))


def splice_bytes(pieces, w, h, channels, error_factor=0, flags=0):
    """pieces: (stream, src_bx, src_by, dst_bx, dst_by, blocks_w, blocks_h) -> the expected stream (numpy uint8); None where the rules refuse the call"""
    parsed = [S.parse(p[0]) for p in pieces]
    geometry = [(int(hd["sizeX"]), int(hd["sizeY"])) + tuple(p[1:7]) for (hd, _, _), p in zip(parsed, pieces)]
    if not accepted(geometry, w, h) or any(int(hd["channels"]) != channels for hd, _, _ in parsed):
        return None
    bx, by = blocks(w), blocks(h)
    owner = np.zeros((by, bx), dtype=np.int64)
    for k, (_, _, sbx, sby, dbx, dby, bw, bh) in enumerate(geometry):
        owner[dby:dby + bh, dbx:dbx + bw] = k
    table = np.zeros(bx * by, dtype=S.BLOCK)
    payload = bytearray()
    for j in range(by):
        for i in range(bx):
            k = int(owner[j, i])
            sw, _, sbx, sby, dbx, dby, _, _ = geometry[k]
            _, src_table, src_payload = parsed[k]
            e = src_table[(sby + j - dby) * blocks(sw) + sbx + i - dbx]
            table[j * bx + i] = e
            table[j * bx + i]["payloadWord"] = len(payload) // 8
            o = int(e["payloadWord"]) * 8
            payload += bytes(src_payload[o:o + 8 * entry_words(e)])
    return S.assemble(S.VERSION, w, h, channels, error_factor, flags, table, payload)


def crop_piece(stream, x, y, w, h):
    """the one piece of a crop; None where the window cannot be cropped (origin not on a block, or an end neither on a block nor on the image's edge)"""
    hd = S.parse(stream)[0]
    W, H = int(hd["sizeX"]), int(hd["sizeY"])
    if w <= 0 or h <= 0 or x + w > W or y + h > H or x % 8 or y % 8 or ((x + w) % 8 and x + w != W) or ((y + h) % 8 and y + h != H):
        return None
    return (stream, x // 8, y // 8, 0, 0, blocks(w), blocks(h))


def crop_bytes(stream, x, y, w, h):
    piece = crop_piece(stream, x, y, w, h)
    if piece is None:
        return None
    hd = S.parse(stream)[0]
    return splice_bytes([piece], w, h, int(hd["channels"]), int(hd["errorFactor"]), int(hd["flags"]))
