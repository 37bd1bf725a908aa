"""Tensor window decode of the version 2 stream (limg_hip_blocked_decode_stream_windows_tensor*): element (c, r, col) of a job is byte c of the pixel of the oracle's
limg_blocked_encode3d_test pDecoded times scale[c] plus bias[c], in float32 or float16, bit for bit what numpy gives for the contract's expression, and nothing else is
written.  A stream with a bad rectangle refuses every job that names it and no other; argument errors, ordering and the host form follow the batched RGBA window decode
(tests/window_tensor.py; the expected pixels never come from the library's own decode)."""
import numpy as np
import pytest

import lib_axis as L
import limg_amd
import window_tensor as T
from oracle import blocked_stream as B
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
    """name -> (img, alpha, pDecoded): computed once, shared, never changed.  The 96 x 72 gradient has merged rectangles of more than 8 blocks; 67 x 45 has partial
    edge blocks both ways."""
    if not _REF:
        for name, img, alpha in (("rg96x72", oracle.random_gradient(96, 72, 3, True), True), ("pn67x45", oracle.photo_noise(67, 45, 3), True),
                                 ("rg64x48", oracle.random_gradient(64, 48, 5, False), True), ("pn256x64", oracle.photo_noise(256, 64, 3), True)):
            got = oracle.blocked_encode3d(img, alpha)
            if name == "rg96x72":
                assert max(int(r["rx"]) * int(r["ry"]) for r in got["regions"]) > 8
            _REF[name] = (img, alpha, got["pDecoded"])
    return _REF


def _stream(gpu, oracle, name):
    """(device stream, nbytes, W, H, pDecoded), and the host bytes"""
    img, alpha, want = _ref(oracle)[name]
    st = gpu.blocked_encode_stream(img, alpha)
    return (device_stream(st), st.size, img.shape[1], img.shape[0], want), st


def _bad_rectangle(st):
    """the largest rectangle moved outside the block grid"""
    hdr, table, _ = B.parse(st)
    evil = st.copy()
    evil[64:64 + 64 * len(table)].view(B.RECT)["ox"][int(np.argmax(table["rx"].astype(int) * table["ry"]))] = int(hdr["blocksX"])
    return evil


@pytest.mark.parametrize("dtype,planes,consts", T.FORMATS)
def test_mixed_batch(gpu, oracle, dtype, planes, consts):
    """every window of windows(W, H) of both images in ONE call: several jobs per stream, so groups form"""
    T.mixed_batch(gpu, gpu.blocked_decode_stream_windows_tensor_device, [_stream(gpu, oracle, n)[0] for n in ("rg96x72", "pn67x45")], dtype, planes, consts)


@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_store_paths_agree(gpu, oracle, dtype):
    T.store_paths_agree(gpu, gpu.blocked_decode_stream_windows_tensor_device, _stream(gpu, oracle, "rg96x72")[0], dtype)


@pytest.mark.parametrize("dtype,planes", [("float32", 3), ("float16", 3), ("float32", 4), ("float16", 4)])
def test_nchw_batch(gpu, oracle, dtype, planes):
    T.nchw_batch(gpu, [_stream(gpu, oracle, n)[0] for n in ("rg96x72", "pn67x45", "rg64x48")], True, dtype, planes)


@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_many_tiny_jobs(gpu, oracle, dtype):
    T.many_tiny_jobs(gpu, gpu.blocked_decode_stream_windows_tensor_device, _stream(gpu, oracle, "pn256x64")[0], dtype)


@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_refusals(gpu, oracle, dtype):
    """a stream with a bad rectangle: every job of that stream writes nothing (bit 1), jobs of another stream in the same call are complete; a header that does not
    match: bit 0; the sticky status reports once"""
    import torch
    (d, nbytes, W, H, want), st = _stream(gpu, oracle, "rg64x48")
    (d2, nbytes2, W2, H2, want2), _ = _stream(gpu, oracle, "pn67x45")
    evil = _bad_rectangle(st)
    magic = st.copy()
    magic[0] ^= 0xFF
    de, dm = device_stream(evil, pad=64 * 64 + 64), device_stream(magic, pad=64 * 64 + 64)
    wins = [(3, 2, 40, 30), (0, 0, 64, 48), (50, 40, 1, 1), (3, 2, 40, 30), (5, 1, 60, 40), (3, 2, 40, 30)]
    streams = [de, de, de, d, d2, dm]
    sizes = [(nbytes, 64, 48)] * 4 + [(nbytes2, W2, H2), (nbytes, 64, 48)]
    fmt = T.fmt_of(dtype, 4, "A")
    outs = [T.sentinel_tensor((4, w[3], w[2] + 3), dtype) for w in wins]
    status = torch.full((len(wins),), 77, dtype=torch.int32, device="cuda")
    gpu.blocked_decode_stream_windows_tensor_device([(s, n, sx, sy, *w, o[1], w[2] + 3, w[3] * (w[2] + 3)) for s, (n, sx, sy), w, o in zip(streams, sizes, wins, outs)],
                                                    fmt, status=status)
    torch.cuda.synchronize()
    with pytest.raises(limg_amd.LimgHipError):
        gpu.check()
    gpu.check()  # reported once
    got = [o[0].cpu().numpy() for o in outs]
    sent = T.SENT[dtype]
    assert all((g == sent).all() for g in got[:3]) and (got[5] == sent).all()
    for g, w, dec in ((got[3], wins[3], want), (got[4], wins[4], want2)):
        assert (g[:, :, w[2]:] == sent).all()
        assert np.array_equal(g[:, :, :w[2]], T.convert(dec[w[1]:w[1] + w[3], w[0]:w[0] + w[2]], dtype, 4, "A").view(T.BITS[dtype]))
    s = status.cpu().tolist()
    assert all(v & 2 for v in s[:3]) and s[3] == 0 and s[4] == 0 and s[5] & 1, s


def test_argument_errors(gpu, oracle):
    (d, nbytes, W, H, want), st = _stream(gpu, oracle, "rg64x48")
    T.argument_errors(gpu, "limg_hip_blocked_decode_stream_windows_tensor_device", d, nbytes, W, H)
    T.host_argument_errors(gpu, "limg_hip_blocked_decode_stream_windows_tensor", st)


def test_back_to_back(gpu, oracle):
    T.back_to_back(gpu, gpu.blocked_decode_stream_windows_tensor_device, _stream(gpu, oracle, "rg96x72")[0])


@pytest.mark.parametrize("dtype,planes,consts", [("float32", 3, "A"), ("float16", 4, "A"), ("float16", 3, "B"), ("float32", 4, "B")])
def test_host_form(gpu, oracle, dtype, planes, consts):
    for name in ("rg96x72", "pn67x45"):
        (d, nbytes, W, H, want), st = _stream(gpu, oracle, name)
        T.host_windows(gpu.blocked_decode_stream_windows_tensor, st, want, windows(W, H), dtype, planes, consts)
    got = gpu.blocked_decode_stream_windows_tensor(st, [(0, 0, W, H)], T.fmt_of(dtype, planes, consts))  # outs=None allocates
    assert np.array_equal(got[0].view(T.BITS[dtype]), T.convert(want, dtype, planes, consts).view(T.BITS[dtype]))
    # a stream that is refused leaves every output untouched
    T.host_windows_refused(gpu.blocked_decode_stream_windows_tensor, _bad_rectangle(st), [(0, 0, 1, 1), (3, 2, 40, 30), (0, 0, W, H)], dtype, planes)
    gpu.check()
    with pytest.raises(limg_amd.LimgHipError):
        gpu.decode_stream_windows_tensor(st, [(0, 0, 8, 8)], T.fmt_of(dtype, planes, consts))  # version 2 bytes given to the version 1 entry
    gpu.check()


L.product_twins(globals())
