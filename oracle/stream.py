"""CPU restatement of the "LMG3" stream container (include/limg_hip.h) -- TEST INFRASTRUCTURE ONLY, like everything under oracle/.

Upstream has no serialised format, so there is no reference bitstream to compare with; what pins this
container is the round trip: `decode(pack(oracle encode))` must equal the pDecoded plane of the reference / oracle bit for bit,
and the GPU packer must produce these exact bytes from the same image.  numpy + per-block calls into the C oracle's a16
(`limg_oracle_block_decode`, src/limg_decode.h:36-236)."""
import numpy as np

MAGIC = 0x33474D4C
VERSION = 1
# (limg_amd carries its own copy of these dtypes for its callers and tests/ compare the two: the restatement stays independent of the product on purpose)
HEADER = np.dtype([("magic", "<u4"), ("version", "<u4"), ("sizeX", "<u4"), ("sizeY", "<u4"), ("channels", "<u4"), ("errorFactor", "<u4"),
                   ("blocksX", "<u4"), ("blocksY", "<u4"), ("payloadWords", "<u8"), ("totalBytes", "<u8"), ("flags", "<u4"), ("reserved", "<u4", 3)])
VECS = ("dirA_min", "dirA_max", "dirB_offset", "dirB_mag", "dirC_offset", "dirC_mag")
ENTRY_FIELDS = [(v, "<i2", 4) for v in VECS] + [("shift", "<u4"), ("payloadWord", "<u4")]  # what a version 1 block entry holds and a version 2 rectangle entry starts with
BLOCK = np.dtype(ENTRY_FIELDS)
assert HEADER.itemsize == 64 and BLOCK.itemsize == 56


# ---- what both versions of the container share (version 2: oracle/blocked_stream.py) ----
def field_bits(shift3, rec, channels):
    """bits per pixel of the three fields and the raw-escape mask (see include/limg_hip.h)."""
    bits, raw = [], 0
    for k in range(3):
        s = int(shift3[k])
        b = 0 if s >= 8 else 8 - s
        if s >= 8 and channels == 4 and int(rec[VECS[2 * k]][3]) != int(rec[VECS[2 * k + 1]][3]):
            b = 8
            raw |= 1 << k
        bits.append(b)
    return bits, raw


def field_words(n, b):
    return (n * b + 63) // 64


def pack_field(values, b):
    """n uint values (< 2**b) -> ceil(n b / 64) words, value i at bit i * b, little endian (an 8x8 block in raster order: pixel (r, x) at bit (8 r + x) * b, 8 b bytes)"""
    acc = 0
    for i, v in enumerate(values.reshape(-1).tolist()):
        acc |= int(v) << (i * b)
    return acc.to_bytes(8 * field_words(values.size, b), "little")


def unpack_field(buf, b, n):
    acc = int.from_bytes(bytes(buf), "little")
    mask = (1 << b) - 1
    return np.array([(acc >> (i * b)) & mask for i in range(n)], dtype=np.uint8)


def fill_entry(e, rec, shift3, raw, payload_word):
    for v in VECS:
        e[v] = rec[v]
    e["shift"] = int(shift3[0]) | (int(shift3[1]) << 8) | (int(shift3[2]) << 16) | (raw << 24)
    e["payloadWord"] = payload_word


def entry_fields(e):
    """table entry -> (record for the oracle's decoder, shift triple, bits per pixel of the three fields, the payload's byte offset)"""
    from .bind import REC_DTYPE
    sw = int(e["shift"])
    shift = [sw & 0xFF, (sw >> 8) & 0xFF, (sw >> 16) & 0xFF]
    rec = np.zeros(1, dtype=REC_DTYPE)
    for v in VECS:
        rec[v] = e[v]
    bits = [8 if (sw >> (24 + k)) & 1 else (0 if shift[k] >= 8 else 8 - shift[k]) for k in range(3)]
    return rec, shift, bits, int(e["payloadWord"]) * 8


def unpack_fields(payload, o, bits, n):
    """the three fields of n pixels each that start at byte o"""
    facs = []
    for b in bits:
        nbytes = 8 * field_words(n, b)
        facs.append(unpack_field(payload[o:o + nbytes], b, n) if b else np.zeros(n, dtype=np.uint8))
        o += nbytes
    return facs


def assemble(version, size_x, size_y, channels, error_factor, flags, table, payload, rectangles=0):
    hdr = np.zeros(1, dtype=HEADER)
    hdr["magic"], hdr["version"] = MAGIC, version
    hdr["sizeX"], hdr["sizeY"], hdr["channels"], hdr["errorFactor"] = size_x, size_y, channels, error_factor
    hdr["blocksX"], hdr["blocksY"] = (size_x + 7) // 8, (size_y + 7) // 8
    hdr["payloadWords"] = len(payload) // 8
    hdr["totalBytes"] = 64 + table.nbytes + len(payload)
    hdr["flags"] = flags
    hdr["reserved"][0][0] = rectangles
    return np.frombuffer(hdr.tobytes() + table.tobytes() + bytes(payload), dtype=np.uint8).copy()


# ---- version 1: one entry per 8x8 block ----
def pack(enc, size_x, size_y, channels, error_factor=100, flags=1):
    """enc: dict from Oracle.encode3d(..., extras=True) (planes + records + shifts + preA/B/C) -> stream bytes (numpy uint8)."""
    bx, by = (size_x + 7) // 8, (size_y + 7) // 8
    table = np.zeros(bx * by, dtype=BLOCK)
    payload = bytearray()
    planes = (enc["pFactorsA"], enc["pFactorsB"], enc["pFactorsC"])
    pres = (enc["preA"], enc["preB"], enc["preC"])
    for j in range(by):
        for i in range(bx):
            rec = enc["records"][j, i]
            sh = enc["shifts"][j, i]
            bits, raw = field_bits(sh, rec, channels)
            fill_entry(table[j * bx + i], rec, sh, raw, len(payload) // 8)
            y0, x0 = j * 8, i * 8
            for k in range(3):
                b = bits[k]
                if b == 0:
                    continue
                grid = np.zeros((8, 8), dtype=np.uint32)
                if (raw >> k) & 1:
                    src = pres[k][y0:y0 + 8, x0:x0 + 8]          # the un-dithered factor byte (what the reference's decoder multiplies at shift 8)
                    grid[:src.shape[0], :src.shape[1]] = src
                else:
                    src = planes[k][y0:y0 + 8, x0:x0 + 8]        # plane byte = value << shift
                    grid[:src.shape[0], :src.shape[1]] = src >> (8 - b)
                payload += pack_field(grid, b)
    return assemble(VERSION, size_x, size_y, channels, error_factor, flags, table, payload)


def parse(stream):
    stream = np.ascontiguousarray(stream, dtype=np.uint8)
    hdr = stream[:64].view(HEADER)[0]
    assert hdr["magic"] == MAGIC and hdr["version"] == VERSION
    n = int(hdr["blocksX"]) * int(hdr["blocksY"])
    table = stream[64:64 + 56 * n].view(BLOCK)
    payload = stream[64 + 56 * n:int(hdr["totalBytes"])]
    return hdr, table, payload


def decode(stream, oracle):
    """stream -> decoded (h, w) uint32 image, a16 per block through the C oracle."""
    hdr, table, payload = parse(stream)
    w, h, ch = int(hdr["sizeX"]), int(hdr["sizeY"]), int(hdr["channels"])
    bx, by = int(hdr["blocksX"]), int(hdr["blocksY"])
    out = np.zeros((h, w), dtype=np.uint32)
    for j in range(by):
        for i in range(bx):
            rec, shift, bits, o = entry_fields(table[j * bx + i])
            rx, ry = min(8, w - i * 8), min(8, h - j * 8)
            # the reference indexes factors by i = yy * rx + xx
            facs = [np.ascontiguousarray(f.reshape(8, 8)[:ry, :rx]).reshape(-1) for f in unpack_fields(payload, o, bits, 64)]
            dec = oracle.block_decode(rx, ry, ch, rec, facs[0], facs[1], facs[2], shift)
            out[j * 8:j * 8 + ry, i * 8:i * 8 + rx] = np.asarray(dec, dtype=np.uint32).reshape(ry, rx)
    return out
