"""Tensor window decode of the version 1 stream (limg_hip_decode_stream_windows_tensor*): element (c, r, col) of a job is byte c of the oracle's pDecoded pixel times
scale[c] plus bias[c], in float32 or float16, bit for bit what numpy gives for the contract's expression -- and nothing else is written: not the row slack, not the gap
between planes, no further plane.  Refused jobs and groups, argument errors, ordering and the host form follow the batched RGBA window decode
(tests/window_tensor.py; the expected pixels never come from the library's own decode)."""
import numpy as np
import pytest

import lib_axis as L
import limg_amd
import window_tensor as T
from oracle import stream as S
from window_batch import device_stream
from window_cases import windows

pytestmark = pytest.mark.gpu


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


_REF = {}


def _ref(oracle):
    """name -> (img, alpha, pDecoded): computed once, shared, never changed.  531 x 19: 67 blocks per row, so two units per block row, ragged both ways."""
    if not _REF:
        for name, img, alpha in (("pn531x19", oracle.photo_noise(531, 19, 3), True), ("rg72x40", oracle.random_gradient(72, 40, 5, True), False),
                                 ("pn64", oracle.photo_noise(64, 64, 3), True), ("pn64b", oracle.photo_noise(64, 64, 9), True),
                                 ("pn256x64", oracle.photo_noise(256, 64, 3), True)):
            _REF[name] = (img, alpha, oracle.encode3d(img, alpha)["pDecoded"])
    return _REF


def _stream(gpu, oracle, name):
    """(device stream, nbytes, W, H, pDecoded), and the host bytes"""
    img, alpha, want = _ref(oracle)[name]
    st = gpu.encode_stream(img, alpha)
    return (device_stream(st), st.size, img.shape[1], img.shape[0], want), st


@pytest.mark.parametrize("dtype,planes,consts", T.FORMATS)
def test_mixed_batch(gpu, oracle, dtype, planes, consts):
    """every window of windows(W, H) of the three images in ONE call; planes = 4 on the 3-channel stream carries byte 3 of the oracle's pixel"""
    T.mixed_batch(gpu, gpu.decode_stream_windows_tensor_device, [_stream(gpu, oracle, n)[0] for n in ("pn531x19", "rg72x40", "pn64")], dtype, planes, consts)


@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_store_paths_agree(gpu, oracle, dtype):
    T.store_paths_agree(gpu, gpu.decode_stream_windows_tensor_device, _stream(gpu, oracle, "pn64")[0], dtype)


@pytest.mark.parametrize("dtype,planes", [("float32", 3), ("float16", 3), ("float32", 4), ("float16", 4)])
def test_nchw_batch(gpu, oracle, dtype, planes):
    T.nchw_batch(gpu, [_stream(gpu, oracle, n)[0] for n in ("rg72x40", "pn64", "pn256x64")], False, dtype, planes)


@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_many_tiny_jobs(gpu, oracle, dtype):
    T.many_tiny_jobs(gpu, gpu.decode_stream_windows_tensor_device, _stream(gpu, oracle, "pn256x64")[0], dtype)


@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_refusals(gpu, oracle, dtype):
    """a corrupted header: the job writes nothing, bit 0; a corrupted payloadWord: its group stores nothing, bit 1, the job's other groups are stored; the jobs around
    them are complete; the sticky status reports once"""
    import torch
    (d, nbytes, W, H, want), st = _stream(gpu, oracle, "pn64")
    (d2, nbytes2, _, _, want2), _ = _stream(gpu, oracle, "pn64b")
    table = len(S.parse(st)[1])
    win = (10, 9, 40, 30)  # blocks 1 .. 6 of block rows 1 .. 4
    evil = st.copy()
    evil[64:64 + 56 * table].view(S.BLOCK)["payloadWord"][2 * 8 + 3] = 0x7FFFFFF0  # block (3, 2): inside the window
    bad = st.copy()
    bad[0] ^= 0xFF
    fmt = T.fmt_of(dtype, 3, "A")
    outs = [T.sentinel_tensor((3, 30, 43), dtype) for _ in range(4)]
    status = torch.full((4,), 77, dtype=torch.int32, device="cuda")
    streams = [(d, nbytes), (device_stream(evil), nbytes), (device_stream(bad), nbytes), (d2, nbytes2)]
    gpu.decode_stream_windows_tensor_device([(s, n, 64, 64, *win, o[1], 43, 30 * 43) for (s, n), o in zip(streams, outs)], fmt, status=status)
    torch.cuda.synchronize()
    with pytest.raises(limg_amd.LimgHipError):
        gpu.check()
    gpu.check()  # reported once
    got = [o[0].cpu().numpy() for o in outs]
    sent = T.SENT[dtype]
    e1, e2 = (T.convert(w[9:39, 10:50], dtype, 3, "A").view(T.BITS[dtype]) for w in (want, want2))
    assert all((g[:, :, 40:] == sent).all() for g in got)
    assert np.array_equal(got[0][:, :, :40], e1) and np.array_equal(got[3][:, :, :40], e2)
    # block row 2 (image rows 16 .. 23) is the refused group
    assert (got[1][:, 7:15] == sent).all() and np.array_equal(got[1][:, :7, :40], e1[:, :7]) and np.array_equal(got[1][:, 15:, :40], e1[:, 15:])
    assert (got[2] == sent).all()
    s = status.cpu().tolist()
    assert s[0] == 0 and s[3] == 0 and s[1] == 2 and s[2] & 1, s
    # every call overwrites the status words: a good list after a refused one
    gpu.decode_stream_windows_tensor_device([(d, nbytes, 64, 64, *win, outs[0][1], 43, 30 * 43)] * 4, fmt, status=status)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0, 0, 0, 0]
    gpu.check()


def test_argument_errors(gpu, oracle):
    (d, nbytes, W, H, want), st = _stream(gpu, oracle, "pn64")
    T.argument_errors(gpu, "limg_hip_decode_stream_windows_tensor_device", d, nbytes, W, H)
    T.host_argument_errors(gpu, "limg_hip_decode_stream_windows_tensor", st)


def test_back_to_back(gpu, oracle):
    T.back_to_back(gpu, gpu.decode_stream_windows_tensor_device, _stream(gpu, oracle, "pn256x64")[0])


@pytest.mark.parametrize("dtype,planes,consts", [("float32", 3, "A"), ("float16", 4, "A"), ("float16", 3, "B"), ("float32", 4, "B")])
def test_host_form(gpu, oracle, dtype, planes, consts):
    for name in ("pn531x19", "rg72x40", "pn64"):
        (d, nbytes, W, H, want), st = _stream(gpu, oracle, name)
        T.host_windows(gpu.decode_stream_windows_tensor, st, want, windows(W, H), dtype, planes, consts)
    got = gpu.decode_stream_windows_tensor(st, [(0, 0, W, H), (5, 3, 9, 2)], T.fmt_of(dtype, planes, consts))  # outs=None allocates
    assert np.array_equal(got[0].view(T.BITS[dtype]), T.convert(want, dtype, planes, consts).view(T.BITS[dtype]))
    assert np.array_equal(got[1].view(T.BITS[dtype]), T.convert(want[3:5, 5:14], dtype, planes, consts).view(T.BITS[dtype]))
    # a stream that is refused for ONE window leaves every output untouched
    evil = st.copy()
    evil[64:64 + 56 * 64].view(S.BLOCK)["payloadWord"][2 * 8 + 3] = 0x7FFFFFF0
    T.host_windows_refused(gpu.decode_stream_windows_tensor, evil, [(0, 0, 8, 8), (10, 9, 40, 30), (56, 56, 8, 8)], dtype, planes)
    gpu.check()
    bad = st.copy()
    bad[0] ^= 0xFF
    T.host_windows_refused(gpu.decode_stream_windows_tensor, bad, [(0, 0, 8, 8)], dtype, planes)
    gpu.check()


L.product_twins(globals())
