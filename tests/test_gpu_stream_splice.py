"""Stream splice (limg_hip_stream_splice*, limg_hip_stream_crop*): a version 1 stream made from rectangles of blocks of version 1 streams on the GPU, without decoding.
The result's BYTES equal what tests/stream_splice_ref.py builds block by block from the sources' bytes, it decodes to the matching rectangles of the sources' decodes
bit for bit, and every rule of the call is refused before anything is written.  Sizes: the smallest that reach each path -- 131 block columns (a run of more than two
chunks of 64), both edges partial, raw-escaped blocks, blocks without payload, 1025 runs (beyond one pass of the scan's 1024)."""
import ctypes as C

import numpy as np
import pytest

import lib_axis as L
import limg_amd
import stream_splice_ref as R
from oracle import stream as S
from window_cases import ERRORS

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A


def _gpu(lib):
    g = L.open_context(lib)
    yield g
    g.check()
    g.close()


@pytest.fixture(scope="module")
def gpu():
    yield from _gpu("test")


@pytest.fixture(scope="module")
def gpu_product():
    yield from _gpu("product")


_cache = {}


def _source(gpu, oracle, name):
    """(stream bytes, its decode), encoded once per library"""
    key = (gpu.library, name)
    if key not in _cache:
        if name == "wide":  # 131 x 5 blocks
            st = gpu.encode_stream(oracle.photo_noise(1048, 40, 5), False)
        elif name == "ragged":  # 33 x 3 blocks, the last column 5 pixels wide, the last row 4 high
            st = gpu.encode_stream(oracle.random_gradient(261, 20, 9, False), True)
        elif name == "tall":  # 2 x 1025 blocks
            st = gpu.encode_stream(oracle.photo_noise(16, 8200, 2), False)
        else:  # forced shifts (8, 8, 8) on the 256 x 32 gradient with varying alpha: with alpha raw-escaped blocks, without it blocks of no payload at all
            gpu.set_options(forced_shift=(8, 8, 8))
            try:
                st = gpu.encode_stream(oracle.random_gradient(256, 32, 21, False), name == "escaped")
            finally:
                gpu.set_options()
        _cache[key] = (st, gpu.decode_stream(st))
    return _cache[key]


def _header(st):
    return S.parse(st)[0]


def _check_crop(gpu, st, full, win):
    """one crop through the host and the device entry: the restatement's bytes, the crop of the source's decode, and a window of the result"""
    import torch
    x, y, w, h = win
    hd = _header(st)
    W, H, alpha = int(hd["sizeX"]), int(hd["sizeY"]), int(hd["channels"]) == 4
    want = R.crop_bytes(st, x, y, w, h)
    assert want is not None, win
    got = gpu.stream_crop(st, x, y, w, h)
    assert np.array_equal(got, want), win
    d = torch.from_numpy(st).cuda()
    out, n = gpu.stream_crop_device(d, st.size, W, H, alpha, x, y, w, h, int(hd["errorFactor"]), int(hd["flags"]))
    assert n == want.size and np.array_equal(out[:n].cpu().numpy(), want), win
    assert limg_amd.stream_info(got, gpu.lib) == (w, h, alpha, want.size)
    assert np.array_equal(gpu.decode_stream(got), full[y:y + h, x:x + w]), win
    ww, wh = max(1, w // 2), max(1, h // 2)  # the window that ends in the crop's last pixel
    assert np.array_equal(gpu.decode_stream_window(got, w - ww, h - wh, ww, wh), full[y + h - wh:y + h, x + w - ww:x + w]), win
    return got


def test_crop_runs_longer_than_two_chunks(gpu, oracle):
    st, full = _source(gpu, oracle, "wide")
    for win in ((0, 0, 1048, 40), (520, 16, 8, 8), (512, 0, 8, 40), (8, 8, 1032, 24), (0, 32, 1048, 8), (1040, 0, 8, 40)):
        _check_crop(gpu, st, full, win)
    assert np.array_equal(gpu.stream_crop(st, 0, 0, 1048, 40), st)  # the whole image: the stream itself
    gpu.check()


def test_crop_with_both_edges_partial(gpu, oracle):
    st, full = _source(gpu, oracle, "ragged")
    for win in ((0, 0, 261, 20), (0, 0, 8, 8), (256, 16, 5, 4), (128, 0, 8, 20), (200, 0, 61, 16), (0, 8, 64, 12), (8, 8, 240, 8), (192, 8, 69, 12)):
        _check_crop(gpu, st, full, win)
    gpu.check()


def test_escapes_and_empty_fields(gpu, oracle):
    st, full = _source(gpu, oracle, "escaped")
    raw = (S.parse(st)[1]["shift"] >> 24).reshape(4, 32)
    assert raw[1:3, 8:24].any(), "the crop below holds no raw-escaped block"
    for win in ((0, 0, 256, 32), (64, 8, 128, 16)):
        got = _check_crop(gpu, st, full, win)
    assert (S.parse(got)[1]["shift"] >> 24).any()
    st, full = _source(gpu, oracle, "empty")
    assert int(_header(st)["payloadWords"]) == 0
    for win in ((0, 0, 256, 32), (64, 8, 128, 16)):
        got = _check_crop(gpu, st, full, win)  # every run's total is 0
    assert got.size == 64 + 56 * 32 and int(_header(got)["payloadWords"]) == 0
    gpu.check()


def test_join_strips(gpu, oracle):
    """the strips of a 264 x 48 image, encoded separately (each restarts the dither chain, as the ranks of a multi-GPU encode do), joined into the image's stream"""
    import torch
    img = oracle.photo_noise(264, 48, 11)
    rows = [(0, 16), (16, 24), (24, 48)]
    strips = [gpu.encode_stream(img[a:b], False) for a, b in rows]
    want_px = np.concatenate([gpu.decode_stream(s) for s in strips])
    joined = gpu.join_strip_streams(strips)
    pieces = [(s, 0, 0, 0, a // 8, 33, (b - a) // 8) for s, (a, b) in zip(strips, rows)]
    hd = _header(strips[0])
    want = R.splice_bytes(pieces, 264, 48, 3, int(hd["errorFactor"]), int(hd["flags"]))
    assert np.array_equal(joined, want)
    assert limg_amd.stream_info(joined, gpu.lib) == (264, 48, False, want.size)
    assert np.array_equal(gpu.decode_stream(joined), want_px)
    assert np.array_equal(gpu.decode_stream_window(joined, 100, 10, 60, 30), want_px[10:40, 100:160])  # across both joins
    # the same on the device, from buffers as limg_hip_gather_stream leaves them
    dev = [(torch.from_numpy(s).cuda(), s.size, 264, b - a) for s, (a, b) in zip(strips, rows)]
    out, n = gpu.join_strip_streams(dev, has_alpha=False)
    assert np.array_equal(out[:n].cpu().numpy(), R.splice_bytes(pieces, 264, 48, 3))
    with pytest.raises(ValueError):
        gpu.join_strip_streams([gpu.encode_stream(img[:12], False), strips[0]])
    gpu.check()


def test_two_by_two_from_four_sources(gpu, oracle):
    """a 261 x 20 image from four streams of four different images: the right-hand tiles bring the partial column, the lower ones the partial row"""
    tiles = [(128, 8, 0, 0), (133, 8, 16, 0), (128, 12, 0, 1), (133, 12, 16, 1)]
    streams = [gpu.encode_stream(oracle.random_gradient(w, h, 30 + i, False), True) for i, (w, h, _, _) in enumerate(tiles)]
    pieces = [(s, 0, 0, dbx, dby, R.blocks(w), R.blocks(h)) for s, (w, h, dbx, dby) in zip(streams, tiles)]
    got = gpu.stream_splice(pieces, 261, 20, True, error_factor=77, flags=3)
    assert np.array_equal(got, R.splice_bytes(pieces, 261, 20, 4, 77, 3))
    px = [gpu.decode_stream(s) for s in streams]
    want_px = np.concatenate([np.concatenate(px[:2], axis=1), np.concatenate(px[2:], axis=1)])
    assert np.array_equal(gpu.decode_stream(got), want_px)
    assert np.array_equal(gpu.decode_stream_window(got, 120, 4, 141, 16), want_px[4:20, 120:261])
    gpu.check()


def test_more_runs_than_one_pass_of_the_scan(gpu, oracle):
    st, full = _source(gpu, oracle, "tall")
    hd = _header(st)
    piece = [(st, 0, 0, 0, 0, 2, 1025)]
    assert len(R.runs([(16, 8200, 0, 0, 0, 0, 2, 1025)], 16, 8200)) == 1025
    got = gpu.stream_splice(piece, 16, 8200, False, int(hd["errorFactor"]), int(hd["flags"]))
    assert np.array_equal(got, R.splice_bytes(piece, 16, 8200, 3, int(hd["errorFactor"]), int(hd["flags"])))
    assert np.array_equal(got, st)
    got = _check_crop(gpu, st, full, (8, 8, 8, 8192))  # 1024 runs of one block, and the last row left out
    gpu.check()


def test_round_trip_is_byte_identical(gpu, oracle):
    """crop into four tiles, splice them back: the source stream, byte for byte"""
    for name, cut_x, cut_y in (("wide", 64, 2), ("ragged", 16, 1)):
        st, _ = _source(gpu, oracle, name)
        hd = _header(st)
        W, H, bx, by = int(hd["sizeX"]), int(hd["sizeY"]), int(hd["blocksX"]), int(hd["blocksY"])
        pieces = []
        for dby, y0, y1 in ((0, 0, 8 * cut_y), (cut_y, 8 * cut_y, H)):
            for dbx, x0, x1 in ((0, 0, 8 * cut_x), (cut_x, 8 * cut_x, W)):
                tile = gpu.stream_crop(st, x0, y0, x1 - x0, y1 - y0)
                pieces.append((tile, 0, 0, dbx, dby, R.blocks(x1 - x0), R.blocks(y1 - y0)))
        back = gpu.stream_splice(pieces, W, H, int(hd["channels"]) == 4, int(hd["errorFactor"]), int(hd["flags"]))
        assert np.array_equal(back, st), name
        assert bx * by == sum(p[5] * p[6] for p in pieces)
    gpu.check()


def _table(pieces):
    return limg_amd.LimgHip._splice_pieces(pieces, False)


def test_host_refusals_write_nothing(gpu, oracle):
    import torch
    st, _ = _source(gpu, oracle, "ragged")  # 33 x 3 blocks of 261 x 20
    sq = gpu.encode_stream(oracle.photo_noise(64, 32, 3), True)  # 8 x 4 blocks
    out = np.full(gpu.stream_bound(264, 32), SENTINEL, dtype=np.uint8)
    n = C.c_size_t(12345)
    left, right = (sq, 0, 0, 0, 0, 4, 4), (sq, 4, 0, 4, 0, 4, 4)

    def call(pieces, w, h, alpha=True, count=None, piece_size=C.sizeof(limg_amd.SplicePiece), capacity=out.size, refused=True):
        table, keep = _table(pieces)
        r = gpu.lib.limg_hip_stream_splice(gpu.ctx, table, len(pieces) if count is None else count, piece_size, w, h, int(alpha), 100, 1, out.ctypes.data, capacity, C.byref(n))
        assert not refused or (out == SENTINEL).all(), (pieces, "a refused call wrote to the output")
        return r

    inv = ERRORS["InvalidParameter"]
    # the accepted call the refusals below are one step from
    assert call([left, right], 64, 32, refused=False) == 0 and n.value == sq.size and np.array_equal(out[:n.value], sq) and (out[n.value:] == SENTINEL).all()
    out[:] = SENTINEL
    assert call([left], 64, 32) == inv                                            # a gap
    assert call([left, right, right], 64, 32) == inv                              # an overlap
    assert call([left, (sq, 3, 0, 3, 0, 5, 4)], 64, 32) == inv                    # an overlap of one column
    assert call([left, (sq, 5, 0, 4, 0, 4, 4)], 64, 32) == inv                    # a piece outside its source
    assert call([left, (sq, 4, 1, 4, 0, 4, 4)], 64, 32) == inv                    # ... in y
    assert call([left, (sq, 4, 0, 5, 0, 4, 4)], 64, 32) == inv                    # a piece outside the output
    assert call([left, (sq, 4, 0, 4, 0, 0, 4)], 64, 32) == inv                    # a zero-size piece
    assert call([left, right], 64, 32, count=0) == inv                            # count == 0
    assert call([left, right], 64, 32, piece_size=C.sizeof(limg_amd.SplicePiece) - 8) == inv  # a struct smaller than this library's
    assert call([left, right], 61, 32) == inv                                     # edge rule, x: a clipped output column from a whole source column
    assert call([left, right], 64, 29) == inv                                     # edge rule, y
    assert call([(st, 0, 0, 0, 0, 33, 3)], 264, 24) == inv                        # edge rule: whole output blocks from the source's clipped column and row
    assert call([(st, 0, 0, 0, 0, 33, 3)], 264, 20) == inv                        # ... x alone
    assert call([(st, 0, 0, 0, 0, 33, 3)], 261, 24) == inv                        # ... y alone
    assert call([(st, 0, 0, 0, 0, 33, 3)], 262, 20) == inv                        # a column clipped otherwise
    assert call([left, right], 0, 32) == inv
    assert call([left + (64, 32), (sq[:64 + 56 * 31], 4, 0, 4, 0, 4, 4, 64, 32)], 64, 32) == inv  # a source shorter than its table
    assert call([left, (None,) + right[1:] + (64, 32)], 64, 32) == ERRORS["ArgumentNull"]
    # a finished stream longer than the caller's buffer: its size is reported, nothing is written
    assert call([left, right], 64, 32, capacity=sq.size - 1) == ERRORS["OutOfBounds"] and n.value == sq.size
    # the crop's own rules, both forms
    for win in ((4, 0, 8, 8), (0, 4, 8, 8), (0, 0, 12, 8), (0, 0, 8, 12), (0, 0, 0, 8), (8, 8, 8, 0), (256, 0, 8, 8), (0, 16, 8, 8), (264, 0, 8, 8)):
        assert gpu.lib.limg_hip_stream_crop(gpu.ctx, st.ctypes.data, st.size, *win, out.ctypes.data, out.size, C.byref(n)) == inv, win
        assert R.crop_piece(st, *win) is None, win
    assert (out == SENTINEL).all()
    # the device form: capacity below the bound, unaligned pointers, an output that overlaps a source
    d = torch.from_numpy(np.concatenate([sq, np.zeros(16 - sq.size % 16, dtype=np.uint8)])).cuda()
    dout = torch.full((gpu.stream_bound(64, 32) + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    bound = gpu.stream_bound(64, 32)
    dl, dr = ((d, sq.size), 0, 0, 0, 0, 4, 4, 64, 32), ((d, sq.size), 4, 0, 4, 0, 4, 4, 64, 32)

    def dcall(pieces, out_ptr, capacity, w=64, h=32):
        table, _ = limg_amd.LimgHip._splice_pieces(pieces, True)
        return gpu.lib.limg_hip_stream_splice_device(gpu.ctx, table, len(pieces), C.sizeof(limg_amd.SplicePiece), w, h, 1, 100, 1, out_ptr, capacity, C.byref(n), gpu._stream())

    assert dcall([dl, dr], dout.data_ptr(), bound - 1) == inv
    assert dcall([dl, dr], dout.data_ptr() + 8, bound) == inv
    assert dcall([dl, ((d[8:], sq.size - 8),) + dr[1:]], dout.data_ptr(), bound) == inv
    assert dcall([dl, dr], d.data_ptr() + 1024, bound) == inv                       # the output begins inside the source
    assert dcall([dl, dr], d.data_ptr() - bound + 16, bound) == inv                 # ... or ends inside it
    assert dcall([dl], dout.data_ptr(), bound) == inv
    assert gpu.lib.limg_hip_stream_crop_device(gpu.ctx, d.data_ptr(), sq.size, 64, 32, 1, 4, 0, 8, 8, 100, 1, dout.data_ptr(), bound, C.byref(n), gpu._stream()) == inv
    torch.cuda.synchronize()
    assert bool((dout == SENTINEL).all())
    assert dcall([dl, dr], dout.data_ptr(), bound) == 0 and n.value == sq.size and np.array_equal(dout[:n.value].cpu().numpy(), sq)
    gpu.check()


def _refused_on_the_device(gpu, st, stated_w, stated_h, win, alpha):
    """a source the kernels refuse, through both forms: InvalidParameter from check(), no size, nothing beyond the header area written"""
    import torch
    x, y, w, h = win
    piece = (x // 8, y // 8, 0, 0, R.blocks(w), R.blocks(h), stated_w, stated_h)
    d = torch.from_numpy(st).cuda()
    out = torch.full((gpu.stream_bound(w, h),), SENTINEL, dtype=torch.uint8, device="cuda")
    _, n = gpu.stream_splice_device([((d, st.size),) + piece], w, h, alpha, out=out)
    assert n == 0
    with pytest.raises(limg_amd.LimgHipError, match="101"):
        gpu.check()
    gpu.check()  # reported once
    got = out.cpu().numpy()
    assert (got[64:] == SENTINEL).all() and int(got[:64].view(S.HEADER)[0]["totalBytes"]) == 0
    host = np.full(gpu.stream_bound(w, h), SENTINEL, dtype=np.uint8)
    with pytest.raises(limg_amd.LimgHipError, match="101"):
        gpu.stream_splice([(st,) + piece], w, h, alpha, out=host)
    assert (host == SENTINEL).all()
    gpu.check()


def test_device_refusals(gpu, oracle):
    st, full = _source(gpu, oracle, "wide")
    win = (0, 0, 64, 16)
    _refused_on_the_device(gpu, st, 1040, 40, win, False)  # the header says 1048 pixels
    _refused_on_the_device(gpu, st, 1048, 40, win, True)   # the header says three channels
    # two neighbouring entries of the run trade their payloadWord: both offsets stay inside the stream, and the run is no longer start + prefix
    table = S.parse(st)[1]
    assert table["payloadWord"][3] != table["payloadWord"][4]
    evil = st.copy()
    words = evil[64:64 + 56 * len(table)].view(S.BLOCK)["payloadWord"]
    words[3], words[4] = int(table["payloadWord"][4]), int(table["payloadWord"][3])
    _refused_on_the_device(gpu, evil, 1048, 40, win, False)
    # ... in the second chunk of a long run, and in the run's last block
    for k in (70, 130):
        evil = st.copy()
        words = evil[64:64 + 56 * len(table)].view(S.BLOCK)["payloadWord"]
        words[131 + k - 1], words[131 + k] = int(table["payloadWord"][131 + k]), int(table["payloadWord"][131 + k - 1])
        assert words[131 + k - 1] != words[131 + k]
        _refused_on_the_device(gpu, evil, 1048, 40, (0, 8, 1048, 8), False)
        _check_crop(gpu, evil, full, (0, 16, 1048, 24))  # the rows below do not read those entries
    # a run that ends beyond the payload the header admits
    evil = st.copy()
    evil[:64].view(S.HEADER)["payloadWords"] = int(table["payloadWord"][131 * 4 + 100])
    _refused_on_the_device(gpu, evil, 1048, 40, (0, 32, 1048, 8), False)
    _check_crop(gpu, st, full, win)  # the context is usable afterwards


def test_async_device_form(gpu, oracle):
    """pBytes = NULL on a caller's stream: nothing waits, and after a synchronisation the header's totalBytes is right"""
    import torch
    st, _ = _source(gpu, oracle, "wide")
    hd = _header(st)
    d = torch.from_numpy(st).cuda()
    want = R.crop_bytes(st, 64, 8, 984, 32)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        outs = [gpu.stream_crop_device(d, st.size, 1048, 40, False, 64, 8, 984, 32, int(hd["errorFactor"]), int(hd["flags"]), want_size=False) for _ in range(3)]
    side.synchronize()
    for out, n in outs:  # (back to back on one context: each call's tables outlive the call before it)
        assert n is None
        got = out.cpu().numpy()
        assert int(got[:64].view(S.HEADER)[0]["totalBytes"]) == want.size
        assert np.array_equal(got[:want.size], want)
    gpu.check()


L.product_twins(globals())
