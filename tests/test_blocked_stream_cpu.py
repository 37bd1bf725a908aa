"""Version 2 of the "LMG3" stream (the merged-block encoder's rectangles) without a GPU: the host-only entries of the library, and the format text itself --
oracle/blocked_stream.py packs the CPU oracle's merged-block encode into the container as include/limg_hip.h describes it and decodes it again; that round trip
equals the oracle's pDecoded, so the format carries everything a decoder needs, the raw-byte escape included."""
import numpy as np
import pytest

import limg_amd

from oracle import blocked_stream as B
from blocked_stream_ref import small_cases, stream_flags


@pytest.fixture(scope="module")
def lib():
    return limg_amd.load_library()


def test_bound(lib):
    for w, h in ((8, 8), (1, 1), (9, 9), (1024, 618), (8192, 8192)):
        blocks = ((w + 7) // 8) * ((h + 7) // 8)
        assert limg_amd.blocked_stream_bound(w, h, lib) == 64 + blocks * 64 + blocks * 192
    assert limg_amd.blocked_stream_bound(0, 8, lib) == 0 and limg_amd.blocked_stream_bound(8, 0, lib) == 0
    assert limg_amd.blocked_stream_bound(0x7FFFFFF9, 8, lib) == 0  # where version 1's bound is 0
    assert lib.limg_hip_stream_bound(8 * 65536, 8) != 0 and limg_amd.blocked_stream_bound(8 * 65536, 8, lib) == 0  # more than 65535 blocks in a dimension
    assert limg_amd.blocked_stream_bound(8 * 65535, 8, lib) == 64 + 65535 * 256
    assert limg_amd.blocked_stream_bound(8, 8 * 65535 + 1, lib) == 0


def _header(w=24, h=16, channels=4, rects=3, payload_words=5, **kw):
    hdr = np.zeros(1, dtype=B.HEADER)
    hdr["magic"], hdr["version"], hdr["sizeX"], hdr["sizeY"], hdr["channels"] = B.MAGIC, B.VERSION, w, h, channels
    hdr["blocksX"], hdr["blocksY"], hdr["payloadWords"], hdr["flags"] = (w + 7) // 8, (h + 7) // 8, payload_words, 1 | B.FLAG_MERGED
    hdr["reserved"][0][0] = rects
    hdr["totalBytes"] = 64 + 64 * rects + 8 * payload_words
    for k, v in kw.items():
        hdr[k] = v
    return hdr.view(np.uint8).copy()


def test_info_on_hand_built_headers(lib):
    assert limg_amd.blocked_stream_info(_header(), lib) == (24, 16, True, 64 + 192 + 40, 3)
    assert limg_amd.blocked_stream_info(_header(w=17, h=9, channels=3, rects=1), lib) == (17, 9, False, 64 + 64 + 40, 1)
    bad = {"magic": dict(magic=0x12345678), "version 1": dict(version=1), "version 3": dict(version=3), "channels": dict(channels=5), "blocksX": dict(blocksX=2),
           "blocksY": dict(blocksY=3), "sizeX": dict(sizeX=0), "flags": dict(flags=1), "totalBytes": dict(totalBytes=1000), "payloadWords": dict(payloadWords=6 * 24 + 1)}
    for what, kw in bad.items():
        with pytest.raises(limg_amd.LimgHipError):
            limg_amd.blocked_stream_info(_header(**kw), lib)
            pytest.fail(what)
    for rects in (0, 7):  # none, more than blocks
        with pytest.raises(limg_amd.LimgHipError):
            limg_amd.blocked_stream_info(_header(rects=rects), lib)
    with pytest.raises(limg_amd.LimgHipError):
        limg_amd.blocked_stream_info(_header()[:63], lib)


def test_each_info_refuses_the_other_version(lib, oracle):
    with pytest.raises(limg_amd.LimgHipError):
        limg_amd.stream_info(_header(), lib)  # limg_hip_stream_info keeps refusing version 2
    from oracle import stream as S
    img = oracle.photo_noise(16, 8, 3)
    v1 = S.pack(oracle.encode3d(img, True, extras=True), 16, 8, 4)
    assert limg_amd.stream_info(v1, lib)[:2] == (16, 8)
    with pytest.raises(limg_amd.LimgHipError):
        limg_amd.blocked_stream_info(v1, lib)


def test_abi_symbols(lib):
    for s in ("limg_hip_blocked_stream_bound", "limg_hip_blocked_encode_stream_device", "limg_hip_blocked_decode_stream_device", "limg_hip_blocked_encode_stream",
              "limg_hip_blocked_decode_stream", "limg_hip_blocked_stream_info", "limg_hip_blocked_last_stream"):
        assert s in limg_amd.ABI_SYMBOLS and hasattr(lib, s), s
    assert limg_amd.STREAM_RECT_DTYPE == B.RECT and limg_amd.STREAM_HEADER_DTYPE == B.HEADER


def test_format_round_trip_on_the_cpu(lib, oracle):
    """decode(pack(oracle encode)) == the oracle's pDecoded over the small shape list and the option cases: the container as written in the header text is complete."""
    escaped = {}
    for name, img, alpha, kw in small_cases(oracle):
        ch = 4 if alpha else 3
        want = oracle.blocked_encode3d(img, alpha, **kw)
        stream, esc = B.pack(want, img, ch, oracle, error_factor=kw.get("error_factor", 100), flags=stream_flags(kw))
        escaped[name] = esc
        h, w = img.shape
        assert limg_amd.blocked_stream_info(stream, lib) == (w, h, alpha, stream.size, len(want["regions"])), name
        assert stream.size <= limg_amd.blocked_stream_bound(w, h, lib), name
        hdr, table, _ = B.parse(stream)
        assert (np.diff(table["payloadWord"].astype(np.int64)) >= 0).all()
        assert np.array_equal(B.decode(stream, oracle), want["pDecoded"]), name
    # the raw escape is exercised: forced shift 8 on an image whose alpha varies is the sure case
    assert escaped["rga-forced888"] > 0 and escaped["rga-ragged-forced888"] > 0, escaped
    assert escaped["rg-64x64-rgb"] == 0
