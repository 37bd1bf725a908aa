"""What the nine public resized window methods of LimgHip hand to the C ABI, without a library and without a GPU, through the recorder of tests/test_window_dispatch.py:
the symbol, the ctypes type and length of the table, every field of every entry (a level of None becomes LIMG_HIP_RESIZE_AUTO), where the format and status pointers
sit, and the list that comes back.  Outputs are strided views, 1-D buffers with a stride of their own, or None."""
import numpy as np
import pytest
import torch

import limg_amd
from test_window_dispatch import FORMATS, PREFIXES, H, W, Recorder, check_format, check_table, g, the_call, val  # noqa: F401 (g: the fixture)

AUTO = limg_amd.RESIZE_AUTO


def device_jobs(planar, dtype):
    """(the method's job tuples, the table entries they must become, the outputs in order: None = allocated by the call)"""
    streams = [torch.zeros(300, dtype=torch.uint8), torch.zeros(500, dtype=torch.uint8)]
    if planar:
        big, flat = torch.zeros((4, 40, 50), dtype=dtype), torch.zeros(20000, dtype=dtype)
        # (x, y, sw, sh, ow, oh, out, strides as given, strides the table must hold)
        rows = [(8, 16, 90, 70, 30, 20, big[:, 3:23, 5:35], (None, None), (50, 2000)), (0, 0, 16, 8, 16, 8, flat, (32, 512), (32, 512)), (1, 2, 5, 3, 11, 6, flat[8:], (None, None), (11, 66)),
                (3, 1, 100, 50, 9, 5, flat, (16, None), (16, 80)), (4, 4, 7, 3, 7, 3, None, (None, None), (7, 21))]
    else:
        big, flat = torch.zeros((40, 50), dtype=torch.int32), torch.zeros(4000, dtype=torch.int32)
        rows = [(8, 16, 90, 70, 30, 20, big[3:23, 5:35], (None,), (50,)), (0, 0, 16, 8, 16, 8, flat, (64,), (64,)), (1, 2, 5, 3, 11, 6, flat[4:], (None,), (11,)),
                (4, 4, 7, 3, 7, 3, None, (None,), (7,))]
    jobs, want, outs = [], [], []
    for i, (x, y, sw, sh, ow, oh, out, given, strides) in enumerate(rows):
        st, level, flags = streams[i % 2], (None, 0, 3, 1, 2)[i], i & 1
        jobs.append((st, st.numel() - 3, W + i, H - i, level, flags, x, y, sw, sh, ow, oh, out) + given)
        want.append([st.data_ptr(), st.numel() - 3, W + i, H - i, x, y, sw, sh, out, *strides, ow, oh, AUTO if level is None else level, flags])
        outs.append(out)
    return jobs, want, outs


@pytest.mark.parametrize("prefix", PREFIXES)
@pytest.mark.parametrize("planar", (False, True))
def test_batched_device(g, prefix, planar):
    name = "decode_stream_windows_resized" + ("_tensor" if planar else "") + "_device"
    struct = limg_amd.ResizedTensorWindowJob if planar else limg_amd.ResizedWindowJob
    for type_name, planes in (FORMATS if planar else ((None, 0),)):
        fmt = limg_amd.tensor_format(type_name, planes, (0.5, 0.25, 2.0), (1.0, -1.0, 0.0)) if planar else None
        dtype = getattr(torch, type_name) if planar else torch.int32
        for status in (None, torch.zeros(8, dtype=torch.int32)):
            jobs, want, outs = device_jobs(planar, dtype)
            got = getattr(g, prefix + name)(jobs, *([fmt] if planar else []), status=status)
            a = the_call(g, "limg_hip_" + prefix + name)
            assert len(got) == len(jobs)
            for i, (o, w) in enumerate(zip(outs, want)):
                ow, oh = w[-4], w[-3]
                if o is None:  # allocated: (oh, ow) int32, or (planes, oh, ow) of the format's type
                    assert tuple(got[i].shape) == ((planes,) if planar else ()) + (oh, ow) and got[i].dtype == dtype and got[i].device == jobs[i][0].device
                else:
                    assert got[i] is o
                w[8] = got[i].data_ptr()
            check_table(a[0], struct, [tuple(w) for w in want])
            assert a[1] == len(jobs)
            if planar:
                check_format(a[2], fmt)
            assert val(a[-2]) == (None if status is None else status.data_ptr()) and a[-1] is None and len(a) == (5 if planar else 4)


@pytest.mark.parametrize("prefix", PREFIXES)
@pytest.mark.parametrize("planar", (False, True))
def test_batched_host(g, prefix, planar):
    name = "decode_stream_windows_resized" + ("_tensor" if planar else "")
    struct = limg_amd.ResizedTensorWindow if planar else limg_amd.ResizedWindow
    stream = np.arange(300, dtype=np.uint8)
    for type_name, planes in (FORMATS if planar else ((None, 0),)):
        fmt = limg_amd.tensor_format(type_name, planes, (0.5, 0.25, 2.0), (1.0, -1.0, 0.0)) if planar else None
        dtype = np.dtype(type_name) if planar else np.dtype(np.uint32)
        if planar:
            big = np.zeros((5, 40, 50), dtype=dtype)
            rows = [(8, 16, 90, 70, 30, 20, big[:, 3:23, 5:35], (50, 2000)), (0, 0, 5, 3, 16, 8, big[1:, ::2, 2:18], (100, 2000)), (4, 4, 7, 3, 7, 3, None, (7, 21))]
        else:
            big = np.zeros((40, 50), dtype=dtype)
            rows = [(8, 16, 90, 70, 30, 20, big[3:23, 5:35], (50,)), (0, 0, 5, 3, 16, 8, big[::2, 2:18], (100,)), (4, 4, 7, 3, 7, 3, None, (7,))]
        wins = [((None, 2, 0)[i], i & 1) + r[:6] for i, r in enumerate(rows)]
        for outs in (None, [r[6] for r in rows]):
            got = getattr(g, prefix + name)(stream, wins, *([fmt] if planar else []), outs=outs)
            a = the_call(g, "limg_hip_" + prefix + name)
            assert (val(a[0]), a[1]) == (stream.ctypes.data, 300) and a[3] == len(rows) and len(a) == (5 if planar else 4)
            want = []
            for i, (x, y, sw, sh, ow, oh, out, strides) in enumerate(rows):
                if outs is None or out is None:
                    assert got[i].shape == ((planes,) if planar else ()) + (oh, ow) and got[i].dtype == dtype
                    strides = (ow, ow * oh) if planar else (ow,)
                else:
                    assert got[i] is out
                want.append((x, y, sw, sh, got[i].ctypes.data) + strides + (ow, oh, (AUTO, 2, 0)[i], i & 1))
            assert len(got) == len(rows)
            check_table(a[2], struct, want)
            if planar:
                check_format(a[4], fmt)


@pytest.mark.parametrize("blocked", (False, True))
def test_crops_device(g, blocked):
    streams = [torch.zeros(300, dtype=torch.uint8), torch.zeros(500, dtype=torch.uint8)]
    rects = [(8, 16, 100, 60), (3, 5, 20, 30), (0, 1, 10, 6)]
    flips = [(True,), (), (False,)]
    jobs = [(streams[i % 2], 290 + i, W + i, H - i) + rects[i] + flips[i] for i in range(3)]
    symbol = "limg_hip_%sdecode_stream_windows_resized_tensor_device" % ("blocked_" if blocked else "")
    for dtype, planes, out, level in ((torch.float16, 3, None, None), (torch.float32, 4, torch.zeros((3, 4, 6, 10), dtype=torch.float32), 2)):
        got = g.decode_crops_resized_device(jobs, 6, 10, dtype, (0.5, 0.25, 2.0), (1.0, -1.0, 0.0), planes=planes, blocked=blocked, out=out, level=level)
        a = the_call(g, symbol)
        assert (got is out if out is not None else True) and tuple(got.shape) == (3, planes, 6, 10) and got.dtype == dtype and got.is_contiguous()
        want = [(streams[i % 2].data_ptr(), 290 + i, W + i, H - i) + rects[i] + (got[i].data_ptr(), 10, 60, 10, 6, AUTO if level is None else level, 1 if i == 0 else 0) for i in range(3)]
        check_table(a[0], limg_amd.ResizedTensorWindowJob, want)
        f = a[2]._obj
        assert type(a[2]).__name__ == "CArgObject" and isinstance(f, limg_amd.TensorFormat)
        assert (f.type, f.planes) == (limg_amd.TENSOR_F16 if dtype == torch.float16 else limg_amd.TENSOR_F32, planes)
        assert tuple(f.scale) == (0.5, 0.25, 2.0, 1.0) and tuple(f.bias) == (1.0, -1.0, 0.0, 0.0)
        assert a[1] == 3 and a[3] is None and a[4] is None and len(a) == 5
