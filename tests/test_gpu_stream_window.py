"""Window decode of the version 1 stream (limg_hip_decode_stream_window*): any pixel rectangle of the image equals the crop of the full decode -- the oracle's pDecoded
plane at small sizes, the plane path on the device at full size -- bit for bit, and nothing but the window is written (tests/window_cases.py)."""
import numpy as np
import pytest

import lib_axis as L
import limg_amd
from oracle import stream as S
from test_gpu_stream import _cases
from window_cases import ERRORS, SENTINEL, blocks_of, device_window, host_window, windows

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


def _name(r):
    return {v: k for k, v in ERRORS.items()}.get(r, r)


def _both_entries(gpu, st, want, wins):
    import torch
    H, W = want.shape
    d = torch.from_numpy(st).cuda()
    for win in wins:
        host_window(gpu.decode_stream_window, st, want, win)
        for unaligned in (False, True):
            device_window(gpu.decode_stream_window_device, d, st.size, W, H, want, win, unaligned)
    gpu.check()


def test_windows_equal_the_crop_and_write_nothing_else(gpu, oracle):
    for name, img, alpha, kw in _cases(oracle):
        want = oracle.encode3d(img, alpha, **kw)["pDecoded"]
        st = gpu.encode_stream(img, alpha, **kw)
        H, W = img.shape
        full = gpu.decode_stream(st)
        assert np.array_equal(full, want), name
        assert np.array_equal(gpu.decode_stream_window(st, 0, 0, W, H), full), name  # the whole image as a window
        wins = windows(W, H)
        if W % 8 or H % 8:
            assert any(x + w == W and y + h == H and (w < W or h < H) for x, y, w, h in wins), name
        _both_entries(gpu, st, want, wins)


def test_forced_shifts(gpu, oracle):
    """(8, 8, 8) on the gradient with varying alpha stores raw-escaped factors: at least one decoded window must have held such a block."""
    img = oracle.random_gradient(256, 32, 21, False)
    saw_escape = False
    for shift in ((8, 8, 8), (0, 0, 0), (7, 8, 1), (3, 0, 8)):
        want = oracle.encode3d(img, True, extras=True, forced_shift=shift)
        ref_stream = S.pack(want, 256, 32, 4)
        gpu.set_options(forced_shift=shift)
        try:
            st = gpu.encode_stream(img, True)
        finally:
            gpu.set_options()
        assert np.array_equal(st, ref_stream), shift
        raw = (S.parse(st)[1]["shift"] >> 24).reshape(4, 32)
        wins = windows(256, 32)
        for win in wins[1:]:  # (not the whole image: a window that is one)
            bx0, by0, bx1, by1 = blocks_of(win)
            saw_escape |= bool(raw[by0:by1 + 1, bx0:bx1 + 1].any())
        _both_entries(gpu, st, want["pDecoded"], wins)
    assert saw_escape


def test_refusals(gpu, oracle):
    import torch
    img = oracle.photo_noise(64, 64, 3)
    st = gpu.encode_stream(img, True)
    want = gpu.decode_stream(st)
    win = (10, 9, 40, 30)  # blocks 1 .. 6 of block rows 1 .. 4

    def refused(s, w=win):
        out = np.full((w[3], w[2] + 3), SENTINEL, dtype=np.uint32)
        with pytest.raises(limg_amd.LimgHipError):
            gpu.decode_stream_window(s, *w, out=out[:, :w[2]])
            pytest.fail("accepted")
        assert (out == SENTINEL).all()
        gpu.check()

    bad = st.copy(); bad[0] ^= 0xFF
    refused(bad)
    refused(st[:100])
    refused(st[:st.size - 8])
    table = len(S.parse(st)[1])
    evil = st.copy()
    evil[64:64 + 56 * table].view(S.BLOCK)["payloadWord"][2 * 8 + 3] = 0x7FFFFFF0  # block (3, 2): inside the window
    refused(evil)
    evil = st.copy()
    evil[64:64 + 56 * table].view(S.BLOCK)["payloadWord"][8:16] = 0xFFFFFFF0  # 32-bit sums of these wrap
    refused(evil)
    # the same through the device entry: reported once, the offending group stores nothing
    d = torch.from_numpy(evil).cuda()
    out = torch.full((30, 40), SENTINEL, dtype=torch.int32, device="cuda")
    gpu.decode_stream_window_device(d, evil.size, 64, 64, *win, out=out)
    torch.cuda.synchronize()
    with pytest.raises(limg_amd.LimgHipError):
        gpu.check()
    gpu.check()
    got = out.cpu().numpy().view(np.uint32)
    assert (got[:7] == SENTINEL).all() and np.array_equal(got[7:], want[16:39, 10:50])  # block row 1 (image rows 9 .. 15) is the refused group
    # a bad entry OUTSIDE the window does not concern it
    evil = st.copy()
    evil[64:64 + 56 * table].view(S.BLOCK)["payloadWord"][7 * 8 + 7] = 0x7FFFFFF0
    host_window(gpu.decode_stream_window, evil, want, win)
    # argument errors
    ok = np.zeros((8, 8), dtype=np.uint32)
    for args, code in (((0, 0, 0, 8), "InvalidParameter"), ((0, 0, 8, 0), "InvalidParameter"), ((60, 0, 8, 8), "OutOfBounds"), ((0, 57, 8, 8), "OutOfBounds"),
                       ((64, 0, 1, 1), "OutOfBounds"), ((0, 0, 65, 1), "OutOfBounds"), ((1 << 63, 0, 1 << 63, 1), "OutOfBounds")):
        r = gpu.lib.limg_hip_decode_stream_window(gpu.ctx, st.ctypes.data, st.size, *args, ok.ctypes.data, max(args[2], 8))
        assert r == ERRORS[code], (args, r)
    assert _name(gpu.lib.limg_hip_decode_stream_window(gpu.ctx, st.ctypes.data, st.size, 0, 0, 8, 8, ok.ctypes.data, 7)) == "InvalidParameter"  # stride < width
    assert _name(gpu.lib.limg_hip_decode_stream_window(gpu.ctx, None, st.size, 0, 0, 8, 8, ok.ctypes.data, 8)) == "ArgumentNull"
    assert _name(gpu.lib.limg_hip_decode_stream_window(gpu.ctx, st.ctypes.data, st.size, 0, 0, 8, 8, None, 8)) == "ArgumentNull"
    s = gpu._stream()
    for args, code in (((0, 0, 0, 8, out.data_ptr(), 40), "InvalidParameter"), ((0, 0, 8, 8, out.data_ptr(), 7), "InvalidParameter"), ((60, 60, 8, 4, out.data_ptr(), 40), "OutOfBounds"),
                       ((0, 0, 8, 8, out.data_ptr() + 2, 40), "InvalidParameter"), ((0, 0, 8, 8, None, 40), "ArgumentNull")):
        assert _name(gpu.lib.limg_hip_decode_stream_window_device(gpu.ctx, d.data_ptr(), st.size, 64, 64, *args, s)) == code, args
    gpu.check()
    host_window(gpu.decode_stream_window, st, want, win)  # the context is usable afterwards


FULL_SIZE_WINDOWS = lambda n: [(0, 0, 1024, 1024), (n - 1024, 0, 1024, 1024), (0, n - 1024, 1024, 1024), (n - 1024, n - 1024, 1024, 1024), (123, 457, 1000, 1000),  # noqa: E731
                               (0, 1003, n, 8), (2501, 0, 8, n)]


def test_full_size_on_the_device(gpu):
    """8192^2 photo-noise and 4096^2 gradient: every window equals that slice of the plane path's pDecoded, on the device."""
    import torch
    for kind, n in (("photo_noise", 8192), ("random_gradient", 4096)):
        img = gpu.synth_device(kind, n, n, seed=1)
        planes = gpu.alloc_planes_device(n, n)
        gpu.encode3d_device(img, True, planes)
        st, nbytes = gpu.encode_stream_device(img, True)
        want = planes["pDecoded"]
        for i, win in enumerate(FULL_SIZE_WINDOWS(n)):
            device_window(gpu.decode_stream_window_device, st, nbytes, n, n, want, win, unaligned=bool(i & 1))
            x, y, w, h = win
            out = gpu.decode_stream_window_device(st, nbytes, n, n, x, y, w, h)
            torch.cuda.synchronize()
            assert torch.equal(out, want[y:y + h, x:x + w]), (kind, win)
        gpu.check()
        del planes, st, img, want
        torch.cuda.empty_cache()


L.product_twins(globals())
