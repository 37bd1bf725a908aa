"""Resized window decode of the version 2 stream (limg_hip_blocked_decode_stream_windows_resized*): any source rectangle to any output size, bilinear on the level-L
image of the pDecoded of the oracle's limg_blocked_encode3d_test by the contract's integer formula (numpy: tests/window_resized.py), optionally mirrored, as packed
RGBA8 or through the tensor conversion, bit for bit, and nothing else is written.  Jobs of one stream form a group whatever their levels, sizes and flips; a stream
with a bad rectangle refuses every job that names it and no other."""
import numpy as np
import pytest

import lib_axis as L
import limg_amd
import window_resized as R
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
# 96 x 72: merged rectangles of more than 8 blocks; 67 x 45: partial edge blocks both ways; 531 x 19 and 72 x 40: the tile test's
IMAGES = {"rg96x72": ("random_gradient", 96, 72, 3, True), "pn67x45": ("photo_noise", 67, 45, 3, True), "rg64x48": ("random_gradient", 64, 48, 5, False),
          "pn168x104": ("photo_noise", 168, 104, 4, True), "pn531x19": ("photo_noise", 531, 19, 3, True), "rg72x40": ("random_gradient", 72, 40, 5, False),
          "pn5x3": ("photo_noise", 5, 3, 2, True)}


def _ref(oracle, name):
    """name -> (img, pyramid of the oracle's pDecoded): computed once, shared, never changed"""
    if name not in _REF:
        kind, w, h, seed, opaque = IMAGES[name]
        img = oracle.photo_noise(w, h, seed) if kind == "photo_noise" else oracle.random_gradient(w, h, seed, opaque)
        _REF[name] = (img, W.pyramid(oracle.blocked_encode3d(img, True)["pDecoded"]))
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
    R.mixed_batch(gpu, True, [_stream(gpu, oracle, n)[0] for n in ("rg96x72", "pn67x45", "rg64x48")], mode)


def test_tiles(gpu, oracle):
    R.tiles(gpu, True, [_stream(gpu, oracle, n)[0] for n in ("rg72x40", "pn531x19")], L.has_hooks(gpu))


def test_identity_pure_level_and_flip(gpu, oracle):
    R.identity_level_flip(gpu, True, [_stream(gpu, oracle, n)[0] for n in ("rg96x72", "pn67x45")])


def test_ragged_and_dropped_edges(gpu, oracle):
    R.ragged_edges(gpu, True, _stream(gpu, oracle, "pn531x19")[0], _stream(gpu, oracle, "pn5x3")[0])


def test_tensor_equals_conversion_of_rgba(gpu, oracle):
    R.tensor_equals_conversion_of_rgba(gpu, True, _stream(gpu, oracle, "rg96x72")[0])


@pytest.mark.parametrize("dtype,planes", [("float16", 3), ("float32", 4)])
def test_crops(gpu, oracle, dtype, planes):
    R.crops(gpu, True, [_stream(gpu, oracle, n)[0] for n in ("pn168x104", "rg96x72", "pn67x45")], dtype, planes)


@pytest.mark.parametrize("mode", ["rgba", ("float16", 4, "A")], ids=W.mode_id)
def test_refusals(gpu, oracle, mode):
    """a stream whose largest rectangle lies outside the grid: every job that names it writes nothing (bit 1), whatever its level, size and flip; the jobs of other
    streams in the same call are complete; a header that does not match: bit 0; the sticky status reports once and a good call clears the words"""
    import torch
    (d, nbytes, _, _, pyr), st = _stream(gpu, oracle, "rg64x48")
    (d2, nbytes2, W2, H2, pyr2), _ = _stream(gpu, oracle, "pn67x45")
    magic = st.copy()
    magic[0] ^= 0xFF
    de, dm = device_stream(_bad_rectangle(st), pad=64 * 64 + 64), device_stream(magic, pad=64 * 64 + 64)
    # (stream, nbytes, W, H, pyramid or None where nothing may be written, level, flip, source rectangle, ow, oh)
    jobs = [(de, nbytes, 64, 48, None, 0, 0, (3, 2, 40, 30), 23, 17), (de, nbytes, 64, 48, None, R.AUTO, 1, (0, 0, 64, 48), 16, 12), (de, nbytes, 64, 48, None, 2, 0, (3, 2, 50, 40), 9, 7),
            (de, nbytes, 64, 48, None, 3, 1, (7, 5, 1, 1), 2, 2), (d, nbytes, 64, 48, pyr, 1, 1, (3, 2, 40, 30), 23, 17), (d2, nbytes2, W2, H2, pyr2, R.AUTO, 0, (1, 1, 60, 40), 15, 9),
            (dm, nbytes, 64, 48, None, 1, 0, (3, 2, 40, 30), 20, 15), (d, nbytes, 64, 48, pyr, 0, 0, (0, 0, 8, 6), 13, 11)]
    status = torch.full((len(jobs),), 77, dtype=torch.int32, device="cuda")
    expect = lambda p, lv, fl, rect, ow, oh: R.resize(p, rect, ow, oh, lv, bool(fl))[0]
    if mode == "rgba":
        outs = [torch.full((j[9], j[8] + 3), SENTINEL, dtype=torch.int32, device="cuda") for j in jobs]
        call = lambda: gpu.blocked_decode_stream_windows_resized_device([(s, n, w, h, lv, fl, *rect, ow, oh, o, ow + 3) for (s, n, w, h, _, lv, fl, rect, ow, oh), o in zip(jobs, outs)],
                                                                        status=status)
        call()
        torch.cuda.synchronize()
        got, sent = [o.cpu().numpy()[None] for o in outs], np.int32(SENTINEL)
        want = lambda *a: expect(*a).view(np.int32)[None]
    else:
        dtype, planes, consts = mode
        pairs = [T.sentinel_tensor((planes, j[9], j[8] + 3), dtype) for j in jobs]
        call = lambda: gpu.blocked_decode_stream_windows_resized_tensor_device(
            [(s, n, w, h, lv, fl, *rect, ow, oh, p[1], ow + 3, oh * (ow + 3)) for (s, n, w, h, _, lv, fl, rect, ow, oh), p in zip(jobs, pairs)], T.fmt_of(dtype, planes, consts), status=status)
        call()
        torch.cuda.synchronize()
        got, sent = [p[0].cpu().numpy() for p in pairs], T.SENT[dtype]
        want = lambda *a: T.convert(expect(*a), dtype, planes, consts).view(T.BITS[dtype])
    with pytest.raises(limg_amd.LimgHipError):
        gpu.check()
    gpu.check()  # reported once
    s = status.cpu().tolist()
    for (_, _, _, _, p, lv, fl, rect, ow, oh), g, code in zip(jobs, got, s):
        if p is None:
            assert (g == sent).all() and code != 0, (lv, rect, code)
        else:
            assert code == 0 and (g[:, :, ow:] == sent).all() and np.array_equal(g[:, :, :ow], want(p, lv, fl, rect, ow, oh)), (lv, rect, code)
    assert all(v & 2 for v in s[:4]) and s[6] & 1, s
    jobs = [jobs[4]] * len(jobs)
    call()
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * len(jobs)
    gpu.check()


def test_argument_errors(gpu, oracle):
    (d, nbytes, w, h, _), st = _stream(gpu, oracle, "rg96x72")
    (dt, tbytes, _, _, _), tiny = _stream(gpu, oracle, "pn5x3")
    R.device_argument_errors(gpu, "limg_hip_blocked_decode_stream_windows_resized_device", False, d, nbytes, w, h, dt, tbytes)
    R.device_argument_errors(gpu, "limg_hip_blocked_decode_stream_windows_resized_tensor_device", True, d, nbytes, w, h, dt, tbytes)
    R.host_argument_errors(gpu, "limg_hip_blocked_decode_stream_windows_resized", False, st, w, h, tiny)
    R.host_argument_errors(gpu, "limg_hip_blocked_decode_stream_windows_resized_tensor", True, st, w, h, tiny)


def test_host_forms(gpu, oracle):
    for name in ("rg96x72", "pn67x45"):
        (_, _, w, h, pyr), st = _stream(gpu, oracle, name)
        R.host_forms(gpu, True, st, w, h, pyr)
    R.host_forms_refused(gpu, True, _bad_rectangle(st), [(0, 0, 0, 0, 8, 8, 5, 5), (R.AUTO, 1, 3, 2, 40, 30, 23, 17), (3, 0, 0, 0, w, h, 4, 3)])
    with pytest.raises(limg_amd.LimgHipError):
        gpu.decode_stream_windows_resized(st, [(0, 0, 0, 0, 8, 8, 8, 8)])  # version 2 bytes given to the version 1 entry
    gpu.check()


def test_back_to_back(gpu, oracle):
    R.back_to_back(gpu, True, _stream(gpu, oracle, "rg64x48")[0])


L.product_twins(globals())
