"""CPU restatement of version 2 of the "LMG3" stream -- the merged-block encoder's rectangles -- written from the format text in include/limg_hip.h, not from the
kernels.  TEST INFRASTRUCTURE ONLY (the version 1 counterpart is oracle/stream.py).

What pins the container: `decode(pack(oracle.blocked_encode3d(img)))` equals the oracle's pDecoded bit for bit on the CPU alone, the GPU packer produces these exact
bytes from the same image, and the GPU decoder turns them back into pDecoded."""
import numpy as np

MAGIC = 0x33474D4C
VERSION = 2
FLAG_MERGED = 4
HEADER = np.dtype([("magic", "<u4"), ("version", "<u4"), ("sizeX", "<u4"), ("sizeY", "<u4"), ("channels", "<u4"), ("errorFactor", "<u4"),
                   ("blocksX", "<u4"), ("blocksY", "<u4"), ("payloadWords", "<u8"), ("totalBytes", "<u8"), ("flags", "<u4"), ("reserved", "<u4", 3)])
RECT = np.dtype([("dirA_min", "<i2", 4), ("dirA_max", "<i2", 4), ("dirB_offset", "<i2", 4), ("dirB_mag", "<i2", 4), ("dirC_offset", "<i2", 4),
                 ("dirC_mag", "<i2", 4), ("shift", "<u4"), ("payloadWord", "<u4"), ("ox", "<u2"), ("oy", "<u2"), ("rx", "<u2"), ("ry", "<u2")])
assert HEADER.itemsize == 64 and RECT.itemsize == 64
VECS = ("dirA_min", "dirA_max", "dirB_offset", "dirB_mag", "dirC_offset", "dirC_mag")
PAIRS = (("dirA_min", "dirA_max"), ("dirB_offset", "dirB_mag"), ("dirC_offset", "dirC_mag"))


def rect_pixels(ox, oy, rx, ry, size_x, size_y):
    """(x0, y0, wpx, hpx) of a rectangle given in 8x8 blocks, clipped to the image"""
    x0, y0 = int(ox) * 8, int(oy) * 8
    return x0, y0, min(int(rx) * 8, size_x - x0), min(int(ry) * 8, size_y - y0)


def field_bits(shift3, rec, channels):
    """bits per pixel of the three fields and the raw-escape mask"""
    bits, raw = [], 0
    for k in range(3):
        s = int(shift3[k])
        b = 0 if s >= 8 else 8 - s
        if s >= 8 and channels == 4 and int(rec[PAIRS[k][0]][3]) != int(rec[PAIRS[k][1]][3]):
            b = 8
            raw |= 1 << k
        bits.append(b)
    return bits, raw


def field_words(n, b):
    return (n * b + 63) // 64


def _pack_field(values, b):
    """n uint values (< 2**b) -> ceil(n b / 64) words, value i at bit i * b, little endian"""
    acc = 0
    for i, v in enumerate(values.reshape(-1).tolist()):
        acc |= int(v) << (i * b)
    return acc.to_bytes(8 * field_words(values.size, b), "little")


def _unpack_field(buf, b, n):
    acc = int.from_bytes(bytes(buf), "little")
    mask = (1 << b) - 1
    return np.array([(acc >> (i * b)) & mask for i in range(n)], dtype=np.uint8)


def pack(want, img, channels, oracle, error_factor=100, flags=1):
    """want: dict from Oracle.blocked_encode3d(img, channels == 4, ...) -> the stream bytes (numpy uint8).  -> (stream, number of escaped fields)"""
    img = np.ascontiguousarray(img, dtype=np.uint32)
    size_y, size_x = img.shape
    bx, by = (size_x + 7) // 8, (size_y + 7) // 8
    regions = want["regions"]
    table = np.zeros(len(regions), dtype=RECT)
    payload = bytearray()
    planes = (want["pFactorsA"], want["pFactorsB"], want["pFactorsC"])
    escaped = 0
    for r, reg in enumerate(regions):
        rec = np.zeros(1, dtype=reg["rec"].dtype)
        rec[0] = reg["rec"]
        bits, raw = field_bits(reg["shift"], rec[0], channels)
        for v in VECS:
            table[r][v] = rec[0][v]
        sh = reg["shift"]
        table[r]["shift"] = int(sh[0]) | (int(sh[1]) << 8) | (int(sh[2]) << 16) | (raw << 24)
        table[r]["payloadWord"] = len(payload) // 8
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
            payload += _pack_field(vals, b)
    hdr = np.zeros(1, dtype=HEADER)
    hdr["magic"], hdr["version"] = MAGIC, VERSION
    hdr["sizeX"], hdr["sizeY"], hdr["channels"], hdr["errorFactor"] = size_x, size_y, channels, error_factor
    hdr["blocksX"], hdr["blocksY"] = bx, by
    hdr["payloadWords"] = len(payload) // 8
    hdr["totalBytes"] = 64 + 64 * len(regions) + len(payload)
    hdr["flags"] = flags | FLAG_MERGED
    hdr["reserved"][0][0] = len(regions)
    return np.frombuffer(hdr.tobytes() + table.tobytes() + bytes(payload), dtype=np.uint8).copy(), escaped


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
    from oracle.bind import REC_DTYPE
    hdr, table, payload = parse(stream)
    w, h, ch = int(hdr["sizeX"]), int(hdr["sizeY"]), int(hdr["channels"])
    out = np.zeros((h, w), dtype=np.uint32)
    covered = np.zeros((h, w), dtype=np.uint8)
    for e in table:
        sw = int(e["shift"])
        shift = [sw & 0xFF, (sw >> 8) & 0xFF, (sw >> 16) & 0xFF]
        raw = sw >> 24
        rec = np.zeros(1, dtype=REC_DTYPE)
        for v in VECS:
            rec[v] = e[v]
        x0, y0, wpx, hpx = rect_pixels(e["ox"], e["oy"], e["rx"], e["ry"], w, h)
        n = wpx * hpx
        o = int(e["payloadWord"]) * 8
        facs = []
        for k in range(3):
            b = 8 if (raw >> k) & 1 else (0 if shift[k] >= 8 else 8 - shift[k])
            nbytes = 8 * field_words(n, b)
            facs.append(_unpack_field(payload[o:o + nbytes], b, n) if b else np.zeros(n, dtype=np.uint8))
            o += nbytes
        dec = oracle.block_decode(wpx, hpx, ch, rec, facs[0], facs[1], facs[2], shift)
        out[y0:y0 + hpx, x0:x0 + wpx] = np.asarray(dec, dtype=np.uint32).reshape(hpx, wpx)
        covered[y0:y0 + hpx, x0:x0 + wpx] += 1
    assert (covered == 1).all(), "every pixel belongs to exactly one rectangle"
    return out


def small_cases(oracle):
    """The shape list of tests/test_gpu_blocked.py::test_stagewise_small plus the option cases of the issue: (name, img, alpha, oracle keywords)."""
    out = []
    for kind, alpha, shape in (("pn", True, (256, 128)), ("rg", True, (256, 128)), ("rga", True, (203, 61)), ("pn", False, (131, 77)), ("rg", False, (64, 64)),
                               ("pn", True, (8, 8)), ("pn", True, (9, 9)), ("rg", False, (17, 10)), ("pn", True, (1, 1)), ("pn", True, (2, 65)), ("pn", False, (25, 33)),
                               ("rg", True, (265, 9)), ("flat", True, (96, 80)), ("flat", True, (200, 168))):
        w, h = shape
        if kind == "flat":
            img = np.full((h, w), 0xFF336699, dtype=np.uint32)
        elif kind == "pn":
            img = oracle.photo_noise(w, h, 5)
        else:
            img = oracle.random_gradient(w, h, 5, kind == "rg")
        out.append(("%s-%dx%d-%s" % (kind, w, h, "rgba" if alpha else "rgb"), img, alpha, {}))
    rga = oracle.random_gradient(128, 64, 3, False)
    for ef in (0, 25, 400):
        out.append(("rga-ef%d" % ef, rga, True, dict(error_factor=ef)))
    out.append(("rga-accurate", rga, True, dict(fast=False)))
    out.append(("pn-accurate-rgb", oracle.photo_noise(72, 40, 7), False, dict(fast=False)))
    out.append(("rga-pcg", rga, True, dict(dither_mode=1)))
    out.append(("pn-pcg-ragged", oracle.photo_noise(75, 41, 7), True, dict(dither_mode=1)))
    for shift in ((8, 8, 8), (0, 0, 0), (3, 5, 8)):
        out.append(("rga-forced%d%d%d" % shift, rga, True, dict(forced_shift=shift)))
    out.append(("rga-ragged-forced888", oracle.random_gradient(75, 41, 3, False), True, dict(forced_shift=(8, 8, 8))))
    ramp = np.zeros((64, 512), dtype=np.uint32)
    ramp[:] = 0xFF000000 | (np.arange(512, dtype=np.uint32)[None, :] // 4) * 0x010101  # a slow horizontal ramp: one very wide rectangle
    out.append(("ramp", ramp, True, {}))
    return out


def stream_flags(kw):
    return (1 if kw.get("fast", True) else 0) | (2 if kw.get("dither_mode", 0) else 0)
