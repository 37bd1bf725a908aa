"""What the public stream error and quality methods of LimgHip hand to the C ABI, without a library and without a GPU: a LimgHip whose `.lib` records every call
(the recorder of tests/test_window_dispatch.py).  For each method: the symbol, the ctypes type and length of the table, every field of every entry, where the sums,
status, limits and results sit, and what comes back."""
import ctypes as C

import numpy as np
import pytest
import torch

import limg_amd
from test_window_dispatch import Recorder, check_table, the_call, val

PREFIXES = ("", "blocked_")
W, H = 200, 120


@pytest.fixture
def g():
    h = object.__new__(limg_amd.LimgHip)
    h.lib = Recorder()
    h.ctx = C.c_void_p()
    h._stream = lambda: None
    h.stream_bound = lambda w, hh: 64 + 248 * ((w + 7) // 8) * ((hh + 7) // 8)
    return h


@pytest.mark.parametrize("prefix", PREFIXES)
def test_error_windows_device(g, prefix):
    streams = [torch.zeros(300, dtype=torch.uint8), torch.zeros(500, dtype=torch.uint8)]
    big, flat = torch.zeros((40, 50), dtype=torch.int32), torch.zeros(2000, dtype=torch.int32)
    view = big[3:3 + 20, 5:5 + 30]
    jobs = [(streams[0], 290, W, H, 7, 9, 30, 20, view, None), (streams[1], 480, W, H, 0, 0, 11, 6, flat, 64), (streams[0], 290, W, H, 1, 2, 11, 6, flat[1:], None)]
    want = [(streams[0].data_ptr(), 290, W, H, 7, 9, 30, 20, view.data_ptr(), 50), (streams[1].data_ptr(), 480, W, H, 0, 0, 11, 6, flat.data_ptr(), 64),
            (streams[0].data_ptr(), 290, W, H, 1, 2, 11, 6, flat[1:].data_ptr(), 11)]
    fn, symbol = getattr(g, prefix + "decode_stream_windows_error_device"), "limg_hip_%sdecode_stream_windows_error_device" % prefix
    sums, status = torch.zeros(3, dtype=torch.int64), torch.zeros(3, dtype=torch.int32)
    got = fn(jobs, sums=sums, status=status)
    a = the_call(g, symbol)
    assert got is sums and len(a) == 5 and a[1] == 3 and (val(a[2]), val(a[3])) == (sums.data_ptr(), status.data_ptr()) and a[4] is None
    check_table(a[0], limg_amd.ErrorWindowJob, want)
    got = fn(jobs)  # sums allocated, no status
    a = the_call(g, symbol)
    assert got.dtype == torch.int64 and tuple(got.shape) == (3,) and val(a[2]) == got.data_ptr() and a[3] is None
    check_table(a[0], limg_amd.ErrorWindowJob, want)


@pytest.mark.parametrize("prefix", PREFIXES)
def test_error_windows_host(g, prefix):
    stream = np.arange(300, dtype=np.uint8)
    big = np.zeros((40, 50), dtype=np.uint32)
    wins = [(7, 9, 30, 20), (1, 2, 11, 6)]
    originals = [big[3:3 + 20, 5:5 + 30], np.zeros((6, 11), dtype=np.uint32)]
    got = getattr(g, prefix + "decode_stream_windows_error")(stream, wins, originals)
    a = the_call(g, "limg_hip_%sdecode_stream_windows_error" % prefix)
    assert got == [0, 0] and (val(a[0]), a[1], a[3]) == (stream.ctypes.data, 300, 2) and len(a) == 5
    check_table(a[2], limg_amd.ErrorWindow, [(7, 9, 30, 20, originals[0].ctypes.data, 50), (1, 2, 11, 6, originals[1].ctypes.data, 11)])
    assert isinstance(a[4], C.Array) and a[4]._type_ is C.c_uint64 and len(a[4]) == 2


def test_stream_compare_and_the_psnr_helper(g):
    stream, original = np.arange(300, dtype=np.uint8), np.zeros((6, 11), dtype=np.uint32)
    g.stream_compare(stream, original)
    a = the_call(g, "limg_hip_stream_compare")
    assert (val(a[0]), a[1], val(a[2]), a[3]) == (stream.ctypes.data, 300, original.ctypes.data, 66) and len(a) == 6
    g.error_sum_for_psnr(11, 6, True, 38)
    name, args = g.lib.calls.pop()
    assert name == "limg_hip_error_sum_for_psnr" and args == (11, 6, 1, 38.0) and isinstance(args[3], float)  # (no context)


def test_quality_single(g):
    img = np.zeros((16, 24), dtype=np.uint32)
    st, res = g.encode_stream_quality(img, True, 12345, 4, 64, pool_threads=2, fast=False)
    a = the_call(g, "limg_hip_encode_stream_quality")
    assert a[1:4] == (24, 16, 1) and a[5] == g.stream_bound(24, 16) and a[6:11] == (12345, 4, 64, 2, 0) and len(a) == 12
    assert a[11]._obj is res and res.struct_size == C.sizeof(limg_amd.QualityResult) == 32 and st.size == 0
    dimg = torch.zeros((16, 24), dtype=torch.int32)
    out, res = g.encode_stream_quality_device(dimg, False, 7)
    a = the_call(g, "limg_hip_encode_stream_quality_device")
    assert (val(a[0]), a[1], a[2], a[3], val(a[4]), a[5]) == (dimg.data_ptr(), 24, 16, 0, out.data_ptr(), out.numel()) and a[6:11] == (7, 0, 0, 0, 1)
    assert a[11]._obj is res and a[12] is None and len(a) == 13 and out.numel() == g.stream_bound(24, 16)


def test_quality_list(g):
    imgs = [np.zeros((16, 24), dtype=np.uint32) for _ in range(3)]
    streams, results = g.encode_stream_quality_batch(imgs, True, [5, 6, 7], 2, 128)
    a = the_call(g, "limg_hip_encode_stream_quality_batch")
    assert a[0] == 3 and a[2:5] == (24, 16, 1) and a[6] == g.stream_bound(24, 16) and list(a[7]) == [5, 6, 7] and a[7]._type_ is C.c_uint64 and a[8:12] == (2, 128, 0, 1)
    assert a[12]._type_ is limg_amd.QualityResult and len(a[12]) == 3 and all(r.struct_size == 32 for r in a[12]) and len(a) == 13
    assert len(streams) == 3 and len(results) == 3
    dimgs = [torch.zeros((16, 24), dtype=torch.int32) for _ in range(2)]
    outs, results = g.encode_stream_quality_batch_device(dimgs, False, 9)
    a = the_call(g, "limg_hip_encode_stream_quality_batch_device")
    assert a[0] == 2 and [v for v in a[1]] == [t.data_ptr() for t in dimgs] and [v for v in a[5]] == [o.data_ptr() for o in outs] and list(a[7]) == [9, 9]
    assert a[13] is None and len(a) == 14 and len(results) == 2
