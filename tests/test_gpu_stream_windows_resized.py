"""Resized window decode of the version 1 stream (limg_hip_decode_stream_windows_resized*): any source rectangle to any output size, bilinear on the level-L image of
the oracle's pDecoded by the contract's integer formula (numpy: tests/window_resized.py), optionally mirrored, as packed RGBA8 or through the tensor conversion, bit for
bit, and nothing else is written.  Levels, sizes and flips mix in one call; identity is the batched window entry, a pure level the scaled entry; tiles of any capacity
give the same pixels; refused headers and groups, argument errors, the host forms and the ring follow the batched window decode."""
import numpy as np
import pytest

import lib_axis as L
import limg_amd
import window_resized as R
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
# the images of the scaled tests: 531 x 19 has 67 blocks per row (two units per block row), is ragged both ways and 66 x 2 at level 3
IMAGES = {"pn531x19": ("photo_noise", 531, 19, 3, True), "rg72x40": ("random_gradient", 72, 40, 5, False), "pn64": ("photo_noise", 64, 64, 3, True),
          "pn64b": ("photo_noise", 64, 64, 9, True), "pn168x104": ("photo_noise", 168, 104, 4, True), "pn5x3": ("photo_noise", 5, 3, 2, True)}


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
    R.mixed_batch(gpu, False, [_stream(gpu, oracle, n)[0] for n in ("pn531x19", "rg72x40", "pn64")], mode)


def test_tiles(gpu, oracle):
    R.tiles(gpu, False, [_stream(gpu, oracle, n)[0] for n in ("rg72x40", "pn531x19")], L.has_hooks(gpu))


def test_identity_pure_level_and_flip(gpu, oracle):
    R.identity_level_flip(gpu, False, [_stream(gpu, oracle, n)[0] for n in ("pn531x19", "rg72x40")])


def test_ragged_and_dropped_edges(gpu, oracle):
    R.ragged_edges(gpu, False, _stream(gpu, oracle, "pn531x19")[0], _stream(gpu, oracle, "pn5x3")[0])


def test_tensor_equals_conversion_of_rgba(gpu, oracle):
    R.tensor_equals_conversion_of_rgba(gpu, False, _stream(gpu, oracle, "pn64")[0])


@pytest.mark.parametrize("dtype,planes", [("float32", 3), ("float16", 4)])
def test_crops(gpu, oracle, dtype, planes):
    R.crops(gpu, False, [_stream(gpu, oracle, n)[0] for n in ("pn168x104", "rg72x40", "pn64")], dtype, planes)


@pytest.mark.parametrize("mode", ["rgba", ("float32", 3, "A")], ids=W.mode_id)
def test_refusals(gpu, oracle, mode):
    """level 0, source (5, 4, 40, 30) of a 64 x 64 image to 23 x 17.  A corrupted header: the job writes nothing, bit 0.  A corrupted payloadWord of block (3, 2) fails the
    group of block row 2 (source rows 16 .. 23): status 2, every output pixel whose two row taps lie outside rows 16 .. 23 is correct, nothing outside the 23 x 17
    rectangle is written.  The jobs around them are complete; the sticky status reports once and a following good call overwrites the status words with 0"""
    import torch
    (d, nbytes, _, _, pyr), st = _stream(gpu, oracle, "pn64")
    (d2, nbytes2, _, _, pyr2), _ = _stream(gpu, oracle, "pn64b")
    table = len(S.parse(st)[1])
    rect, ow, oh = (5, 4, 40, 30), 23, 17
    evil = st.copy()
    evil[64:64 + 56 * table].view(S.BLOCK)["payloadWord"][2 * 8 + 3] = 0x7FFFFFF0
    bad = st.copy()
    bad[0] ^= 0xFF
    streams = [(d, nbytes), (device_stream(bad), nbytes), (device_stream(evil), nbytes), (d2, nbytes2)]
    status = torch.full((4,), 77, dtype=torch.int32, device="cuda")
    w1, w2 = (R.resize(p, rect, ow, oh, 0, False)[0] for p in (pyr, pyr2))
    if mode == "rgba":
        outs = [torch.full((oh, ow + 3), SENTINEL, dtype=torch.int32, device="cuda") for _ in range(4)]
        call = lambda jobs: gpu.decode_stream_windows_resized_device([(s, n, 64, 64, 0, 0, *rect, ow, oh, o, ow + 3) for (s, n), o in jobs], status=status)
        call(zip(streams, outs))
        e1, e2 = w1.view(np.int32)[None], w2.view(np.int32)[None]
        got, sent = [o.cpu().numpy()[None] for o in outs], np.int32(SENTINEL)
    else:
        dtype, planes, consts = mode
        fmt = T.fmt_of(dtype, planes, consts)
        pairs = [T.sentinel_tensor((planes, oh, ow + 3), dtype) for _ in range(4)]
        outs = [p[1] for p in pairs]
        call = lambda jobs: gpu.decode_stream_windows_resized_tensor_device([(s, n, 64, 64, 0, 0, *rect, ow, oh, o, ow + 3, oh * (ow + 3)) for (s, n), o in jobs], fmt, status=status)
        call(zip(streams, outs))
        e1, e2 = (T.convert(w, dtype, planes, consts).view(T.BITS[dtype]) for w in (w1, w2))
        got, sent = [p[0].cpu().numpy() for p in pairs], T.SENT[dtype]
    torch.cuda.synchronize()
    with pytest.raises(limg_amd.LimgHipError):
        gpu.check()
    gpu.check()  # reported once
    assert all((g[:, :, ow:] == sent).all() for g in got)
    assert np.array_equal(got[0][:, :, :ow], e1) and np.array_equal(got[3][:, :, :ow], e2)
    assert (got[1] == sent).all()
    ya, yb, _ = R.axis(rect[1], rect[3], oh, 0, 64)
    sound = ~(((ya >= 16) & (ya <= 23)) | ((yb >= 16) & (yb <= 23)))  # output rows with no tap in the failed group
    assert 0 < int(sound.sum()) < oh
    assert np.array_equal(got[2][:, sound, :ow], e1[:, sound])
    s = status.cpu().tolist()
    assert s[0] == 0 and s[3] == 0 and s[2] == 2 and s[1] & 1, s
    call([(streams[0], outs[0])] * 4)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0, 0, 0, 0]
    gpu.check()


def test_argument_errors(gpu, oracle):
    (d, nbytes, w, h, _), st = _stream(gpu, oracle, "pn64")
    (dt, tbytes, _, _, _), tiny = _stream(gpu, oracle, "pn5x3")
    R.device_argument_errors(gpu, "limg_hip_decode_stream_windows_resized_device", False, d, nbytes, w, h, dt, tbytes)
    R.device_argument_errors(gpu, "limg_hip_decode_stream_windows_resized_tensor_device", True, d, nbytes, w, h, dt, tbytes)
    R.host_argument_errors(gpu, "limg_hip_decode_stream_windows_resized", False, st, w, h, tiny)
    R.host_argument_errors(gpu, "limg_hip_decode_stream_windows_resized_tensor", True, st, w, h, tiny)


def test_host_forms(gpu, oracle):
    for name in ("pn531x19", "pn64"):
        (_, _, w, h, pyr), st = _stream(gpu, oracle, name)
        R.host_forms(gpu, False, st, w, h, pyr)
    evil = st.copy()
    evil[64:64 + 56 * 64].view(S.BLOCK)["payloadWord"][2 * 8 + 3] = 0x7FFFFFF0  # block (3, 2): inside the footprint of the second window only
    R.host_forms_refused(gpu, False, evil, [(0, 0, 0, 0, 8, 8, 5, 5), (0, 1, 10, 8, 40, 30, 23, 17), (3, 0, 56, 56, 8, 8, 1, 1)])
    bad = st.copy()
    bad[0] ^= 0xFF
    R.host_forms_refused(gpu, False, bad, [(R.AUTO, 0, 0, 0, 64, 64, 16, 16)])


def test_back_to_back(gpu, oracle):
    R.back_to_back(gpu, False, _stream(gpu, oracle, "rg72x40")[0])


L.product_twins(globals())
