"""What the 22 public window methods of LimgHip hand to the C ABI, without a library and without a GPU: a LimgHip whose `.lib` records every call.  For each method:
the symbol, the ctypes type and length of the table, every field of every entry, where the format and status pointers sit, and the list that comes back.  Outputs are
strided views, 1-D buffers with a stride of their own, or None; the scaled forms mix levels."""
import ctypes as C

import numpy as np
import pytest
import torch

import limg_amd
from limg_amd import LimgHip


class Recorder:
    """stands in for the loaded library: any attribute is a function that notes (symbol, arguments) and reports success"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


@pytest.fixture
def g():
    h = object.__new__(LimgHip)
    h.lib = Recorder()
    h.ctx = C.c_void_p()
    h._stream = lambda: None
    return h


def val(a):
    """a pointer argument as a number (None stays None)"""
    return a.value if isinstance(a, C.c_void_p) else a


def the_call(g, symbol):
    assert len(g.lib.calls) == 1, g.lib.calls
    name, args = g.lib.calls.pop()
    assert name == symbol
    assert args[0] is g.ctx
    return args[1:]


def fields(s):
    return tuple(getattr(s, k) for k, _ in s._fields_)


def check_table(table, struct, want):
    assert isinstance(table, C.Array) and table._type_ is struct and len(table) == len(want)
    for got, w in zip(table, want):
        if hasattr(got, "window"):  # a job: pStream, streamBytes, sizeX, sizeY, then the window's x0, y0, width, height, pOut, strides, level
            assert fields(got)[:4] + fields(got.window) == w
        else:
            assert fields(got) == w


def check_format(arg, fmt):
    assert type(arg).__name__ == "CArgObject" and arg._obj is fmt  # C.byref(fmt)


PREFIXES = ("", "blocked_")
FORMATS = (("float32", 3), ("float16", 4))
W, H = 200, 120  # the image the device jobs state


# ---- the 4 single-window methods ----
@pytest.mark.parametrize("prefix", PREFIXES)
def test_single_window_host(g, prefix):
    stream = np.arange(300, dtype=np.uint8)
    big = np.zeros((40, 50), dtype=np.uint32)
    out = big[3:3 + 20, 5:5 + 30]
    got = getattr(g, prefix + "decode_stream_window")(stream, 7, 9, 30, 20, out=out)
    a = the_call(g, "limg_hip_%sdecode_stream_window" % prefix)
    assert got is out
    assert (val(a[0]), a[1]) == (stream.ctypes.data, 300) and a[2:6] == (7, 9, 30, 20) and (val(a[6]), a[7]) == (out.ctypes.data, 50) and len(a) == 8
    got = getattr(g, prefix + "decode_stream_window")(stream, 1, 2, 11, 6)
    a = the_call(g, "limg_hip_%sdecode_stream_window" % prefix)
    assert got.shape == (6, 11) and got.dtype == np.uint32
    assert a[2:6] == (1, 2, 11, 6) and (val(a[6]), a[7]) == (got.ctypes.data, 11)


@pytest.mark.parametrize("prefix", PREFIXES)
def test_single_window_device(g, prefix):
    stream = torch.zeros(300, dtype=torch.uint8)
    big = torch.zeros((40, 50), dtype=torch.int32)
    view, flat = big[3:3 + 20, 5:5 + 30], torch.zeros(2000, dtype=torch.int32)
    fn, symbol = getattr(g, prefix + "decode_stream_window_device"), "limg_hip_%sdecode_stream_window_device" % prefix
    for out, out_stride, stride in ((view, None, 50), (flat, 64, 64), (flat, None, 30)):
        got = fn(stream, 290, W, H, 7, 9, 30, 20, out=out, out_stride=out_stride)
        a = the_call(g, symbol)
        assert got is out
        assert (val(a[0]), a[1]) == (stream.data_ptr(), 290) and a[2:8] == (W, H, 7, 9, 30, 20) and (val(a[8]), a[9]) == (out.data_ptr(), stride) and a[10] is None and len(a) == 11
    got = fn(stream, 290, W, H, 1, 2, 11, 6)
    a = the_call(g, symbol)
    assert tuple(got.shape) == (6, 11) and got.dtype == torch.int32 and (val(a[8]), a[9]) == (got.data_ptr(), 11)


# ---- the 16 batched methods ----
def device_jobs(scaled, planar, dtype):
    """(the method's job tuples, the table entries they must become, the outputs in order: None = allocated by the call)"""
    streams = [torch.zeros(300, dtype=torch.uint8), torch.zeros(500, dtype=torch.uint8)]
    if planar:
        big = torch.zeros((4, 40, 50), dtype=dtype)
        flat = torch.zeros(20000, dtype=dtype)
        # (x, y, w, h, out, strides as given, strides the table must hold)
        rows = [(8, 16, 30, 20, big[:, 3:23, 5:35], (None, None), (50, 2000)), (0, 0, 16, 8, flat, (32, 512), (32, 512)), (1, 2, 11, 6, flat[8:], (None, None), (11, 66)),
                (3, 1, 9, 5, flat, (16, None), (16, 80)), (4, 4, 7, 3, None, (None, None), (7, 21))]
    else:
        big = torch.zeros((40, 50), dtype=torch.int32)
        flat = torch.zeros(4000, dtype=torch.int32)
        rows = [(8, 16, 30, 20, big[3:23, 5:35], (None,), (50,)), (0, 0, 16, 8, flat, (64,), (64,)), (1, 2, 11, 6, flat[4:], (None,), (11,)), (4, 4, 7, 3, None, (None,), (7,))]
    jobs, want, outs = [], [], []
    for i, (x, y, w, h, out, given, strides) in enumerate(rows):
        st, level = streams[i % 2], (i + 1) % 4
        jobs.append((st, st.numel() - 3, W + i, H - i) + ((level,) if scaled else ()) + (x, y, w, h, out) + given)
        want.append([st.data_ptr(), st.numel() - 3, W + i, H - i, x, y, w, h, out, *strides] + ([level] if scaled else []))
        outs.append(out)
    return jobs, want, outs


@pytest.mark.parametrize("prefix", PREFIXES)
@pytest.mark.parametrize("scaled", (False, True))
@pytest.mark.parametrize("planar", (False, True))
def test_batched_device(g, prefix, scaled, planar):
    name = "decode_stream_windows" + ("_scaled" if scaled else "") + ("_tensor" if planar else "") + "_device"
    struct = {(False, False): limg_amd.WindowJob, (False, True): limg_amd.TensorWindowJob, (True, False): limg_amd.ScaledWindowJob,
              (True, True): limg_amd.ScaledTensorWindowJob}[scaled, planar]
    for type_name, planes in (FORMATS if planar else ((None, 0),)):
        fmt = limg_amd.tensor_format(type_name, planes, (0.5, 0.25, 2.0), (1.0, -1.0, 0.0)) if planar else None
        dtype = getattr(torch, type_name) if planar else torch.int32
        for status in (None, torch.zeros(8, dtype=torch.int32)):
            jobs, want, outs = device_jobs(scaled, planar, dtype)
            got = getattr(g, prefix + name)(jobs, *([fmt] if planar else []), status=status)
            a = the_call(g, "limg_hip_" + prefix + name)
            assert len(got) == len(jobs)
            for i, (o, w) in enumerate(zip(outs, want)):
                if o is None:  # allocated: (h, w) int32, or (planes, h, w) of the format's type
                    assert tuple(got[i].shape) == ((planes,) if planar else ()) + (w[7], w[6]) and got[i].dtype == dtype and got[i].device == jobs[i][0].device
                else:
                    assert got[i] is o
                w[8] = got[i].data_ptr()
            check_table(a[0], struct, [tuple(w) for w in want])
            assert a[1] == len(jobs)
            if planar:
                check_format(a[2], fmt)
            assert val(a[-2]) == (None if status is None else status.data_ptr()) and a[-1] is None and len(a) == (5 if planar else 4)


@pytest.mark.parametrize("prefix", PREFIXES)
@pytest.mark.parametrize("scaled", (False, True))
@pytest.mark.parametrize("planar", (False, True))
def test_batched_host(g, prefix, scaled, planar):
    name = "decode_stream_windows" + ("_scaled" if scaled else "") + ("_tensor" if planar else "")
    struct = {(False, False): limg_amd.Window, (False, True): limg_amd.TensorWindow, (True, False): limg_amd.ScaledWindow, (True, True): limg_amd.ScaledTensorWindow}[scaled, planar]
    stream = np.arange(300, dtype=np.uint8)
    for type_name, planes in (FORMATS if planar else ((None, 0),)):
        fmt = limg_amd.tensor_format(type_name, planes, (0.5, 0.25, 2.0), (1.0, -1.0, 0.0)) if planar else None
        dtype = np.dtype(type_name) if planar else np.dtype(np.uint32)
        if planar:
            big = np.zeros((5, 40, 50), dtype=dtype)
            rows = [(8, 16, 30, 20, big[:, 3:23, 5:35], (50, 2000)), (0, 0, 16, 8, big[1:, ::2, 2:18], (100, 2000)), (4, 4, 7, 3, None, (7, 21))]
        else:
            big = np.zeros((40, 50), dtype=dtype)
            rows = [(8, 16, 30, 20, big[3:23, 5:35], (50,)), (0, 0, 16, 8, big[::2, 2:18], (100,)), (4, 4, 7, 3, None, (7,))]
        wins = [((i + 2) % 4,) * scaled + r[:4] for i, r in enumerate(rows)]
        for outs in (None, [r[4] for r in rows]):
            got = getattr(g, prefix + name)(stream, wins, *([fmt] if planar else []), outs=outs)
            a = the_call(g, "limg_hip_" + prefix + name)
            assert (val(a[0]), a[1]) == (stream.ctypes.data, 300) and a[3] == len(rows) and len(a) == (5 if planar else 4)
            want = []
            for i, (x, y, w, h, out, strides) in enumerate(rows):
                if outs is None or out is None:
                    assert got[i].shape == ((planes,) if planar else ()) + (h, w) and got[i].dtype == dtype
                    strides = (w, w * h) if planar else (w,)
                else:
                    assert got[i] is out
                want.append((x, y, w, h, got[i].ctypes.data) + strides + (((i + 2) % 4,) if scaled else ()))
            assert len(got) == len(rows)
            check_table(a[2], struct, want)
            if planar:
                check_format(a[4], fmt)


# ---- the 2 crops methods ----
@pytest.mark.parametrize("blocked", (False, True))
@pytest.mark.parametrize("scaled", (False, True))
def test_crops_device(g, blocked, scaled):
    streams = [torch.zeros(300, dtype=torch.uint8), torch.zeros(500, dtype=torch.uint8)]
    at = [(8, 16), (3, 5), (0, 1)]
    jobs = [(streams[i % 2], 290 + i, W + i, H - i) + (((i + 1) % 4,) if scaled else ()) + at[i] for i in range(3)]
    fn = g.decode_crops_scaled_device if scaled else g.decode_crops_device
    symbol = "limg_hip_%sdecode_stream_windows_%stensor_device" % ("blocked_" if blocked else "", "scaled_" if scaled else "")
    struct = limg_amd.ScaledTensorWindowJob if scaled else limg_amd.TensorWindowJob
    for dtype, planes, out in ((torch.float16, 3, None), (torch.float32, 4, torch.zeros((3, 4, 6, 10), dtype=torch.float32))):
        got = fn(jobs, 6, 10, dtype, (0.5, 0.25, 2.0), (1.0, -1.0, 0.0), planes=planes, blocked=blocked, out=out)
        a = the_call(g, symbol)
        assert (got is out if out is not None else True) and tuple(got.shape) == (3, planes, 6, 10) and got.dtype == dtype and got.is_contiguous()
        want = [(streams[i % 2].data_ptr(), 290 + i, W + i, H - i) + at[i] + (10, 6, got[i].data_ptr(), 10, 60) + (((i + 1) % 4,) if scaled else ()) for i in range(3)]
        check_table(a[0], struct, want)
        f = a[2]._obj
        assert type(a[2]).__name__ == "CArgObject" and isinstance(f, limg_amd.TensorFormat)
        assert (f.type, f.planes) == (limg_amd.TENSOR_F16 if dtype == torch.float16 else limg_amd.TENSOR_F32, planes)
        assert tuple(f.scale) == (0.5, 0.25, 2.0, 1.0) and tuple(f.bias) == (1.0, -1.0, 0.0, 0.0)
        assert a[1] == 3 and a[3] is None and a[4] is None and len(a) == 5
