"""Reduced-scale window decode of the version 1 stream (limg_hip_decode_stream_windows_scaled*): pixel (X, Y) of level L is, byte by byte, the rounded mean of the
(1 << L)^2 box of the oracle's pDecoded at ((X << L), (Y << L)) -- reduced in numpy by the contract's integer formula (tests/window_scaled.py) -- as packed RGBA8 or
through the tensor conversion, bit for bit, and nothing else is written.  All levels mix in one call; level 0 is the existing entry; refused groups and jobs, argument
errors, the host forms and the ring follow the batched window decode."""
import numpy as np
import pytest

import lib_axis as L
import limg_amd
import window_scaled as W
import window_tensor as T
from oracle import stream as S
from window_batch import device_stream
from window_cases import SENTINEL

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


_REF, _STREAMS = {}, {}
# 531 x 19: 67 blocks per row, so two units per block row, ragged both ways, level 3 is 66 x 2; the last three: level 3 holds a 20 x 12 crop
IMAGES = {"pn531x19": ("photo_noise", 531, 19, 3, True), "rg72x40": ("random_gradient", 72, 40, 5, False), "pn64": ("photo_noise", 64, 64, 3, True),
          "pn64b": ("photo_noise", 64, 64, 9, True), "pn168x104": ("photo_noise", 168, 104, 4, True), "rg160x96": ("random_gradient", 160, 96, 6, False),
          "pn176x100": ("photo_noise", 176, 100, 8, True), "pn5x3": ("photo_noise", 5, 3, 2, True)}


def _ref(oracle, name):
    """name -> (img, alpha, pyramid of the oracle's pDecoded): computed once, shared, never changed"""
    if name not in _REF:
        kind, w, h, seed, alpha = IMAGES[name]
        img = oracle.photo_noise(w, h, seed) if kind == "photo_noise" else oracle.random_gradient(w, h, seed, True)
        _REF[name] = (img, alpha, W.pyramid(oracle.encode3d(img, alpha)["pDecoded"]))
    return _REF[name]


def _stream(gpu, oracle, name):
    """(device stream, nbytes, W, H, pyramid), and the host bytes; one encode per library"""
    key = (gpu.library, name)
    if key not in _STREAMS:
        img, alpha, pyr = _ref(oracle, name)
        st = gpu.encode_stream(img, alpha)
        _STREAMS[key] = ((device_stream(st), st.size, img.shape[1], img.shape[0], pyr), st)
    return _STREAMS[key]


@pytest.mark.parametrize("mode", W.MODES, ids=W.mode_id)
def test_mixed_batch(gpu, oracle, mode):
    W.mixed_batch(gpu, False, [_stream(gpu, oracle, n)[0] for n in ("pn531x19", "rg72x40", "pn64")], mode)


def test_level0_equals_the_existing_entry(gpu, oracle):
    W.level0_equals_existing(gpu, False, [_stream(gpu, oracle, n)[0] for n in ("pn531x19", "rg72x40")])


def test_tensor_equals_conversion_of_rgba(gpu, oracle):
    W.tensor_equals_conversion_of_rgba(gpu, False, _stream(gpu, oracle, "pn64")[0])


@pytest.mark.parametrize("dtype,planes", [("float32", 3), ("float16", 3), ("float32", 4), ("float16", 4)])
def test_crops(gpu, oracle, dtype, planes):
    W.crops(gpu, False, [_stream(gpu, oracle, n)[0] for n in ("pn168x104", "rg160x96", "pn176x100")], dtype, planes)


@pytest.mark.parametrize("mode", ["rgba", ("float32", 3, "A")], ids=W.mode_id)
def test_refusals(gpu, oracle, mode):
    """level 1, window (5, 4, 20, 15): source footprint (10, 8, 40, 30), block rows 1 .. 4.  A corrupted header: the job writes nothing, bit 0; a corrupted payloadWord of
    block (3, 2): window rows 4 .. 7 (source rows 16 .. 23) keep the sentinel, the other rows are correct, status 2; the jobs around them are complete; the sticky status
    reports once and a following good call overwrites the status words with 0"""
    import torch
    (d, nbytes, _, _, pyr), st = _stream(gpu, oracle, "pn64")
    (d2, nbytes2, _, _, pyr2), _ = _stream(gpu, oracle, "pn64b")
    table = len(S.parse(st)[1])
    win = (5, 4, 20, 15)
    evil = st.copy()
    evil[64:64 + 56 * table].view(S.BLOCK)["payloadWord"][2 * 8 + 3] = 0x7FFFFFF0
    bad = st.copy()
    bad[0] ^= 0xFF
    streams = [(d, nbytes), (device_stream(bad), nbytes), (device_stream(evil), nbytes), (d2, nbytes2)]
    status = torch.full((4,), 77, dtype=torch.int32, device="cuda")
    if mode == "rgba":
        outs = [torch.full((15, 23), SENTINEL, dtype=torch.int32, device="cuda") for _ in range(4)]
        call = lambda jobs: gpu.decode_stream_windows_scaled_device([(s, n, 64, 64, 1, *win, o, 23) for (s, n), o in jobs], status=status)
        call(zip(streams, outs))
        e1, e2 = (p[1][4:19, 5:25].view(np.int32)[None] for p in (pyr, pyr2))
        got, sent = [o.cpu().numpy()[None] for o in outs], np.int32(SENTINEL)
    else:
        dtype, planes, consts = mode
        fmt = T.fmt_of(dtype, planes, consts)
        pairs = [T.sentinel_tensor((planes, 15, 23), dtype) for _ in range(4)]
        outs = [p[1] for p in pairs]
        call = lambda jobs: gpu.decode_stream_windows_scaled_tensor_device([(s, n, 64, 64, 1, *win, o, 23, 15 * 23) for (s, n), o in jobs], fmt, status=status)
        call(zip(streams, outs))
        e1, e2 = (T.convert(p[1][4:19, 5:25], dtype, planes, consts).view(T.BITS[dtype]) for p in (pyr, pyr2))
        got, sent = [p[0].cpu().numpy() for p in pairs], T.SENT[dtype]
    torch.cuda.synchronize()
    with pytest.raises(limg_amd.LimgHipError):
        gpu.check()
    gpu.check()  # reported once
    assert all((g[:, :, 20:] == sent).all() for g in got)
    assert np.array_equal(got[0][:, :, :20], e1) and np.array_equal(got[3][:, :, :20], e2)
    assert (got[1] == sent).all()
    assert (got[2][:, 4:8] == sent).all() and np.array_equal(got[2][:, :4, :20], e1[:, :4]) and np.array_equal(got[2][:, 8:, :20], e1[:, 8:])
    s = status.cpu().tolist()
    assert s[0] == 0 and s[3] == 0 and s[2] == 2 and s[1] & 1, s
    call([(streams[0], outs[0])] * 4)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0, 0, 0, 0]
    gpu.check()


def test_argument_errors(gpu, oracle):
    (d, nbytes, w, h, _), st = _stream(gpu, oracle, "pn64")
    (dt, tbytes, _, _, _), tiny = _stream(gpu, oracle, "pn5x3")
    W.device_argument_errors(gpu, "limg_hip_decode_stream_windows_scaled_device", False, d, nbytes, w, h, dt, tbytes)
    W.host_argument_errors(gpu, "limg_hip_decode_stream_windows_scaled_tensor", True, st, w, h, tiny)


def test_host_forms(gpu, oracle):
    for name in ("pn531x19", "pn64"):  # (531 x 19: level 3 is 66 x 2)
        (_, _, w, h, pyr), st = _stream(gpu, oracle, name)
        W.host_forms(gpu, False, st, w, h, pyr)
    evil = st.copy()
    evil[64:64 + 56 * 64].view(S.BLOCK)["payloadWord"][2 * 8 + 3] = 0x7FFFFFF0  # block (3, 2): inside the footprint of the second window only
    W.host_forms_refused(gpu, False, evil, [(0, 0, 0, 8, 8), (1, 5, 4, 20, 15), (3, 7, 7, 1, 1)])
    bad = st.copy()
    bad[0] ^= 0xFF
    W.host_forms_refused(gpu, False, bad, [(2, 0, 0, 4, 4)])


def test_back_to_back(gpu, oracle):
    W.back_to_back(gpu, False, _stream(gpu, oracle, "rg72x40")[0])


L.product_twins(globals())
