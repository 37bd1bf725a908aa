"""Reduced-scale window decode of the version 2 stream (limg_hip_blocked_decode_stream_windows_scaled*): pixel (X, Y) of level L is, byte by byte, the rounded mean of
the (1 << L)^2 box of the pDecoded of the oracle's limg_blocked_encode3d_test at ((X << L), (Y << L)) -- reduced in numpy by the contract's integer formula
(tests/window_scaled.py) -- as packed RGBA8 or through the tensor conversion, bit for bit, and nothing else is written.  All levels mix in one call and jobs of one
stream form a group whatever their levels; a stream with a bad rectangle refuses every job that names it, at every level, and no other."""
import numpy as np
import pytest

import lib_axis as L
import limg_amd
import window_scaled as W
import window_tensor as T
from oracle import blocked_stream as B
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
# 96 x 72: merged rectangles of more than 8 blocks; 67 x 45: partial edge blocks both ways, and the dropped trailing rows and columns differ per level; the last three:
# level 3 holds a 20 x 12 crop
IMAGES = {"rg96x72": ("random_gradient", 96, 72, 3, True), "pn67x45": ("photo_noise", 67, 45, 3, True), "rg64x48": ("random_gradient", 64, 48, 5, False),
          "pn168x104": ("photo_noise", 168, 104, 4, True), "rg160x96": ("random_gradient", 160, 96, 6, True), "rg176x100": ("random_gradient", 176, 100, 8, False),
          "pn5x3": ("photo_noise", 5, 3, 2, True)}


def _ref(oracle, name):
    """name -> (img, pyramid of the oracle's pDecoded): computed once, shared, never changed"""
    if name not in _REF:
        kind, w, h, seed, opaque = IMAGES[name]
        img = oracle.photo_noise(w, h, seed) if kind == "photo_noise" else oracle.random_gradient(w, h, seed, opaque)
        got = oracle.blocked_encode3d(img, True)
        if name == "rg96x72":
            assert max(int(r["rx"]) * int(r["ry"]) for r in got["regions"]) > 8
        _REF[name] = (img, W.pyramid(got["pDecoded"]))
    return _REF[name]


def _stream(gpu, oracle, name):
    """(device stream, nbytes, W, H, pyramid), and the host bytes; one encode per library"""
    key = (gpu.library, name)
    if key not in _STREAMS:
        img, pyr = _ref(oracle, name)
        st = gpu.blocked_encode_stream(img, True)
        _STREAMS[key] = ((device_stream(st), st.size, img.shape[1], img.shape[0], pyr), st)
    return _STREAMS[key]


def _bad_rectangle(st):
    """the largest rectangle moved outside the block grid"""
    hdr, table, _ = B.parse(st)
    evil = st.copy()
    evil[64:64 + 64 * len(table)].view(B.RECT)["ox"][int(np.argmax(table["rx"].astype(int) * table["ry"]))] = int(hdr["blocksX"])
    return evil


@pytest.mark.parametrize("mode", W.MODES, ids=W.mode_id)
def test_mixed_batch(gpu, oracle, mode):
    W.mixed_batch(gpu, True, [_stream(gpu, oracle, n)[0] for n in ("rg96x72", "pn67x45", "rg64x48")], mode)


def test_level0_equals_the_existing_entry(gpu, oracle):
    W.level0_equals_existing(gpu, True, [_stream(gpu, oracle, n)[0] for n in ("rg96x72", "pn67x45")])


def test_tensor_equals_conversion_of_rgba(gpu, oracle):
    W.tensor_equals_conversion_of_rgba(gpu, True, _stream(gpu, oracle, "rg96x72")[0])


@pytest.mark.parametrize("dtype,planes", [("float32", 3), ("float16", 3), ("float32", 4), ("float16", 4)])
def test_crops(gpu, oracle, dtype, planes):
    W.crops(gpu, True, [_stream(gpu, oracle, n)[0] for n in ("pn168x104", "rg160x96", "rg176x100")], dtype, planes)


@pytest.mark.parametrize("mode", ["rgba", ("float16", 4, "A")], ids=W.mode_id)
def test_refusals(gpu, oracle, mode):
    """a stream whose largest rectangle lies outside the grid: every job that names it writes nothing (bit 1), at every level; the jobs of other streams in the same
    call are complete; a header that does not match: bit 0; the sticky status reports once"""
    import torch
    (d, nbytes, _, _, pyr), st = _stream(gpu, oracle, "rg64x48")
    (d2, nbytes2, W2, H2, pyr2), _ = _stream(gpu, oracle, "pn67x45")
    magic = st.copy()
    magic[0] ^= 0xFF
    de, dm = device_stream(_bad_rectangle(st), pad=64 * 64 + 64), device_stream(magic, pad=64 * 64 + 64)
    # (stream, nbytes, W, H, pyramid or None where nothing may be written, level, window)
    jobs = [(de, nbytes, 64, 48, None, 0, (3, 2, 40, 30)), (de, nbytes, 64, 48, None, 1, (0, 0, 32, 24)), (de, nbytes, 64, 48, None, 2, (3, 2, 9, 7)),
            (de, nbytes, 64, 48, None, 3, (7, 5, 1, 1)), (d, nbytes, 64, 48, pyr, 1, (3, 2, 20, 15)), (d2, nbytes2, W2, H2, pyr2, 2, (1, 1, 15, 9)),
            (dm, nbytes, 64, 48, None, 1, (3, 2, 20, 15)), (d, nbytes, 64, 48, pyr, 3, (0, 0, 8, 6))]
    status = torch.full((len(jobs),), 77, dtype=torch.int32, device="cuda")
    if mode == "rgba":
        outs = [torch.full((j[6][3], j[6][2] + 3), SENTINEL, dtype=torch.int32, device="cuda") for j in jobs]
        gpu.blocked_decode_stream_windows_scaled_device([(s, n, w, h, lv, *win, o, win[2] + 3) for (s, n, w, h, _, lv, win), o in zip(jobs, outs)], status=status)
        torch.cuda.synchronize()
        got, sent = [o.cpu().numpy()[None] for o in outs], np.int32(SENTINEL)
        want = lambda p, lv, win: p[lv][win[1]:win[1] + win[3], win[0]:win[0] + win[2]].view(np.int32)[None]
    else:
        dtype, planes, consts = mode
        pairs = [T.sentinel_tensor((planes, j[6][3], j[6][2] + 3), dtype) for j in jobs]
        gpu.blocked_decode_stream_windows_scaled_tensor_device([(s, n, w, h, lv, *win, p[1], win[2] + 3, win[3] * (win[2] + 3)) for (s, n, w, h, _, lv, win), p in zip(jobs, pairs)],
                                                               T.fmt_of(dtype, planes, consts), status=status)
        torch.cuda.synchronize()
        got, sent = [p[0].cpu().numpy() for p in pairs], T.SENT[dtype]
        want = lambda p, lv, win: T.convert(p[lv][win[1]:win[1] + win[3], win[0]:win[0] + win[2]], dtype, planes, consts).view(T.BITS[dtype])
    with pytest.raises(limg_amd.LimgHipError):
        gpu.check()
    gpu.check()  # reported once
    s = status.cpu().tolist()
    for (_, _, _, _, p, lv, win), g, code in zip(jobs, got, s):
        if p is None:
            assert (g == sent).all() and code != 0, (lv, win, code)
        else:
            assert code == 0 and (g[:, :, win[2]:] == sent).all() and np.array_equal(g[:, :, :win[2]], want(p, lv, win)), (lv, win, code)
    assert all(v & 2 for v in s[:4]) and s[6] & 1, s


def test_argument_errors(gpu, oracle):
    (d, nbytes, w, h, _), st = _stream(gpu, oracle, "rg64x48")
    (dt, tbytes, _, _, _), tiny = _stream(gpu, oracle, "pn5x3")
    W.device_argument_errors(gpu, "limg_hip_blocked_decode_stream_windows_scaled_tensor_device", True, d, nbytes, w, h, dt, tbytes)
    W.host_argument_errors(gpu, "limg_hip_blocked_decode_stream_windows_scaled", False, st, w, h, tiny)


def test_host_forms(gpu, oracle):
    for name in ("rg96x72", "pn67x45"):
        (_, _, w, h, pyr), st = _stream(gpu, oracle, name)
        W.host_forms(gpu, True, st, w, h, pyr)
    W.host_forms_refused(gpu, True, _bad_rectangle(st), [(0, 0, 0, 1, 1), (1, 3, 2, 20, 15), (3, 0, 0, w >> 3, h >> 3)])
    with pytest.raises(limg_amd.LimgHipError):
        gpu.decode_stream_windows_scaled(st, [(1, 0, 0, 8, 8)])  # version 2 bytes given to the version 1 entry
    gpu.check()


def test_back_to_back(gpu, oracle):
    W.back_to_back(gpu, True, _stream(gpu, oracle, "rg96x72")[0])


L.product_twins(globals())
