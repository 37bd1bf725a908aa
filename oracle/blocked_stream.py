"""CPU restatement of version 2 of the "LMG3" stream -- the merged-block encoder's rectangles -- written from the format text in include/limg_hip.h, not from the
kernels.  TEST INFRASTRUCTURE ONLY.  What it shares with version 1 (header, vectors, field widths, entry unpacking, field packer) is oracle/stream.py's.

What pins the container: `decode(pack(oracle.blocked_encode3d(img)))` equals the oracle's pDecoded bit for bit on the CPU alone, the GPU packer produces these exact
bytes from the same image, and the GPU decoder turns them back into pDecoded."""
import numpy as np

from .stream import ENTRY_FIELDS, HEADER, MAGIC, assemble, entry_fields, field_bits, fill_entry, pack_field, unpack_fields  # noqa: F401 (HEADER, MAGIC: for the tests)

VERSION = 2
FLAG_MERGED = 4
RECT = np.dtype(ENTRY_FIELDS + [("ox", "<u2"), ("oy", "<u2"), ("rx", "<u2"), ("ry", "<u2")])
assert RECT.itemsize == 64


def rect_pixels(ox, oy, rx, ry, size_x, size_y):
    """(x0, y0, wpx, hpx) of a rectangle given in 8x8 blocks, clipped to the image"""
    x0, y0 = int(ox) * 8, int(oy) * 8
    return x0, y0, min(int(rx) * 8, size_x - x0), min(int(ry) * 8, size_y - y0)


def pack(want, img, channels, oracle, error_factor=100, flags=1):
    """want: dict from Oracle.blocked_encode3d(img, channels == 4, ...) -> the stream bytes (numpy uint8).  -> (stream, number of escaped fields)"""
    img = np.ascontiguousarray(img, dtype=np.uint32)
    size_y, size_x = img.shape
    regions = want["regions"]
    table = np.zeros(len(regions), dtype=RECT)
    payload = bytearray()
    planes = (want["pFactorsA"], want["pFactorsB"], want["pFactorsC"])
    escaped = 0
    for r, reg in enumerate(regions):
        rec = np.zeros(1, dtype=reg["rec"].dtype)
        rec[0] = reg["rec"]
        bits, raw = field_bits(reg["shift"], rec[0], channels)
        fill_entry(table[r], rec[0], reg["shift"], raw, len(payload) // 8)
        table[r]["ox"], table[r]["oy"], table[r]["rx"], table[r]["ry"] = reg["ox"], reg["oy"], reg["rx"], reg["ry"]
        x0, y0, wpx, hpx = rect_pixels(reg["ox"], reg["oy"], reg["rx"], reg["ry"], size_x, size_y)
        pre = None
        for k in range(3):
            b = bits[k]
            if b == 0:
                continue
            if (raw >> k) & 1:
                if pre is None:  # the un-dithered factor bytes of the rectangle's pixels under its record (the reference skips the dither at shift 8)
                    pre = oracle.block_factors(img[y0:y0 + hpx, x0:x0 + wpx], channels, rec)
                vals = np.asarray(pre[k], dtype=np.uint32)
                escaped += 1
            else:
                vals = planes[k][y0:y0 + hpx, x0:x0 + wpx].astype(np.uint32) >> (8 - b)  # plane byte = value << shift
            payload += pack_field(vals, b)
    return assemble(VERSION, size_x, size_y, channels, error_factor, flags | FLAG_MERGED, table, payload, rectangles=len(regions)), escaped


def parse(stream):
    stream = np.ascontiguousarray(stream, dtype=np.uint8)
    hdr = stream[:64].view(HEADER)[0]
    assert hdr["magic"] == MAGIC and hdr["version"] == VERSION and int(hdr["flags"]) & FLAG_MERGED
    n = int(hdr["reserved"][0])
    assert int(hdr["totalBytes"]) == 64 + 64 * n + 8 * int(hdr["payloadWords"]) and stream.size >= int(hdr["totalBytes"])
    table = stream[64:64 + 64 * n].view(RECT)
    payload = stream[64 + 64 * n:int(hdr["totalBytes"])]
    return hdr, table, payload


def decode(stream, oracle):
    """stream -> decoded (h, w) uint32 image: per rectangle the reference's decoder (a16) through the C oracle, which takes any rectangle size"""
    hdr, table, payload = parse(stream)
    w, h, ch = int(hdr["sizeX"]), int(hdr["sizeY"]), int(hdr["channels"])
    out = np.zeros((h, w), dtype=np.uint32)
    covered = np.zeros((h, w), dtype=np.uint8)
    for e in table:
        rec, shift, bits, o = entry_fields(e)
        x0, y0, wpx, hpx = rect_pixels(e["ox"], e["oy"], e["rx"], e["ry"], w, h)
        facs = unpack_fields(payload, o, bits, wpx * hpx)
        dec = oracle.block_decode(wpx, hpx, ch, rec, facs[0], facs[1], facs[2], shift)
        out[y0:y0 + hpx, x0:x0 + wpx] = np.asarray(dec, dtype=np.uint32).reshape(hpx, wpx)
        covered[y0:y0 + hpx, x0:x0 + wpx] += 1
    assert (covered == 1).all(), "every pixel belongs to exactly one rectangle"
    return out
