"""Window decode of the version 2 stream (limg_hip_blocked_decode_stream_window*): any pixel rectangle equals the crop of the full decode -- the oracle's
limg_blocked_encode3d_test pDecoded at small sizes, the plane path on the device at full size -- bit for bit, nothing but the window is written
(tests/window_cases.py), and a table that is malformed where the window looks is refused with the output untouched."""
import numpy as np
import pytest

import lib_axis as L
import limg_amd
from oracle import blocked_stream as B
from blocked_stream_ref import small_cases
from test_gpu_blocked_stream import _encode
from test_gpu_stream_window import FULL_SIZE_WINDOWS
from window_cases import SENTINEL, blocks_of, device_window, host_window, windows

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


def _inside(regions, W, H):
    """A window that starts and ends strictly inside the largest rectangle of more than one block in each direction, and cuts more than one block of it in each
    direction; None without one."""
    big = [r for r in regions if r["rx"] >= 2 and r["ry"] >= 2]
    if not big:
        return None
    r = max(big, key=lambda r: int(r["rx"]) * int(r["ry"]))
    x, y = int(r["ox"]) * 8 + 3, int(r["oy"]) * 8 + 2
    x1, y1 = min(W, (int(r["ox"]) + int(r["rx"])) * 8) - 2, min(H, (int(r["oy"]) + int(r["ry"])) * 8) - 3
    win = (x, y, x1 - x, y1 - y)
    bx0, by0, bx1, by1 = blocks_of(win)
    if bx1 <= bx0 or by1 <= by0:  # (a rectangle of two blocks whose second is a sliver of a partial edge block)
        return None
    assert bx0 == r["ox"] and by0 == r["oy"] and bx1 < r["ox"] + r["rx"] and by1 < r["oy"] + r["ry"]
    assert x > r["ox"] * 8 and y > r["oy"] * 8 and x1 < (r["ox"] + r["rx"]) * 8 and y1 < (r["oy"] + r["ry"]) * 8
    return win


def _both_entries(gpu, st, want, wins):
    import torch
    H, W = want.shape
    d = torch.zeros(st.size + 64, dtype=torch.uint8, device="cuda")
    d[:st.size] = torch.from_numpy(st).cuda()
    for win in wins:
        host_window(gpu.blocked_decode_stream_window, st, want, win)
        for unaligned in (False, True):
            device_window(gpu.blocked_decode_stream_window_device, d, st.size, W, H, want, win, unaligned)
    gpu.check()


def test_windows_equal_the_crop_and_write_nothing_else(gpu, oracle):
    cut = 0
    for name, img, alpha, kw in small_cases(oracle):
        want = oracle.blocked_encode3d(img, alpha, **kw)["pDecoded"]
        st = _encode(gpu, img, alpha, kw)
        H, W = img.shape
        full = gpu.blocked_decode_stream(st)
        assert np.array_equal(full, want), name
        assert np.array_equal(gpu.blocked_decode_stream_window(st, 0, 0, W, H), full), name  # the whole image as a window
        wins = windows(W, H)
        if W % 8 or H % 8:
            assert any(x + w == W and y + h == H for x, y, w, h in wins[1:]), name
        inside = _inside(gpu.blocked_regions(), W, H)
        if inside:
            wins.append(inside)
            cut += 1
        _both_entries(gpu, st, want, wins)
    assert cut >= 3


def test_window_that_cuts_a_rectangle(gpu, oracle):
    """The gradient has rectangles of several blocks in each direction (a property of the data, checked on the CPU first); a window that starts and ends strictly inside one."""
    img = oracle.random_gradient(256, 128, 5, True)
    want = oracle.blocked_encode3d(img, True)
    assert _inside(want["regions"], 256, 128) is not None
    st = gpu.blocked_encode_stream(img, True)
    win = _inside(gpu.blocked_regions(), 256, 128)
    assert win is not None and win == _inside(want["regions"], 256, 128)
    _both_entries(gpu, st, want["pDecoded"], [win, (win[0] + 8, win[1] + 8, 1, 1), (win[0], win[1], win[2], 1)])


def _mutations(oracle, gpu):
    """Every mutation touches a rectangle that intersects the window: the window is the inside of the largest rectangle."""
    img = oracle.random_gradient(64, 48, 5, False)
    good = gpu.blocked_encode_stream(img, True)
    hdr, table, _ = B.parse(good)
    n = len(table)
    big = int(np.argmax(table["rx"].astype(int) * table["ry"]))
    assert 3 <= n < 48 and table["rx"][big] >= 2 and table["ry"][big] >= 2
    win = _inside(table, 64, 48)
    other = (big + 1) % n
    v1 = gpu.encode_stream(img, True)

    def edit(fn):
        s = good.copy()
        fn(s[:64].view(B.HEADER), s[64:64 + 64 * n].view(B.RECT), s)
        return s

    def place(t, i, ox, oy, rx, ry):
        t["ox"][i], t["oy"][i], t["rx"][i], t["ry"][i] = ox, oy, rx, ry

    padded = np.concatenate([good, np.zeros(64 * 64, np.uint8)])
    ph = padded[:64].view(B.HEADER)
    ph["reserved"][0][0] = 49  # blocks = 48
    ph["totalBytes"] = int(ph["totalBytes"][0]) + 64 * (49 - n)
    b = table[big]
    cases = {
        "wrong magic": edit(lambda h, t, s: h.__setitem__("magic", 0x12345678)),
        "version 1 bytes": v1,
        "truncated table": good[:64 + 64 * (n - 1)],
        "R > blocks": padded,
        "rect outside": edit(lambda h, t, s: t["ox"].__setitem__(big, 8)),
        "payloadWord past the end": edit(lambda h, t, s: t["payloadWord"].__setitem__(big, int(h["payloadWords"][0]) + 1)),
        "overlap": edit(lambda h, t, s: place(t, other, b["ox"], b["oy"], b["rx"], b["ry"])),
        "one block uncovered": edit(lambda h, t, s: t["rx"].__setitem__(big, int(b["rx"]) - 1)),
        # only the window can tell: one block inside it claimed a second time (what `other` leaves uncovered lies outside the window) ...
        "window block claimed twice": edit(lambda h, t, s: place(t, other, b["ox"] + 1, b["oy"] + 1, 1, 1)),
        # ... and one block inside it claimed by nobody: the largest rectangle loses its last block row
        "window block claimed by nobody": edit(lambda h, t, s: t["ry"].__setitem__(big, int(b["ry"]) - 1)),
    }
    return img, good, win, cases


def test_malformed_streams_are_refused(gpu, oracle):
    img, good, win, cases = _mutations(oracle, gpu)
    want = oracle.blocked_encode3d(img, True)["pDecoded"]
    assert len(cases) == 10
    for name, s in cases.items():
        out = np.full((win[3], win[2] + 3), SENTINEL, dtype=np.uint32)
        with pytest.raises(limg_amd.LimgHipError):
            gpu.blocked_decode_stream_window(s, *win, out=out[:, :win[2]])
            pytest.fail("accepted: " + name)
        assert (out == SENTINEL).all(), name
        gpu.check()  # reported once
        host_window(gpu.blocked_decode_stream_window, good, want, win)  # the context decodes correctly afterwards
    with pytest.raises(limg_amd.LimgHipError):
        gpu.decode_stream_window(good, *win)  # version 2 bytes given to the version 1 window decoder


def test_malformed_streams_on_the_device_entry(gpu, oracle):
    """The kernels' own refusal paths: the device entry does no host-side header check; pOut is left untouched and limg_hip_check_device_status reports it once."""
    import torch
    img, good, win, cases = _mutations(oracle, gpu)
    h, w = img.shape
    want = oracle.blocked_encode3d(img, True)["pDecoded"]
    for name, s in cases.items():
        buf = torch.zeros(good.size + 64 * 64 + 64, dtype=torch.uint8, device="cuda")
        buf[:s.size] = torch.from_numpy(s).cuda()
        out = torch.full((win[3], win[2] + 4), SENTINEL, dtype=torch.int32, device="cuda")
        gpu.blocked_decode_stream_window_device(buf, s.size, w, h, *win, out=out)
        with pytest.raises(limg_amd.LimgHipError):
            gpu.check()
            pytest.fail("accepted: " + name)
        gpu.check()
        assert bool((out == SENTINEL).all()), name
        buf[:good.size] = torch.from_numpy(good).cuda()
        device_window(gpu.blocked_decode_stream_window_device, buf, good.size, w, h, want, win, unaligned=False)
        gpu.check()


def test_argument_errors(gpu, oracle):
    from window_cases import ERRORS
    img = oracle.photo_noise(64, 64, 3)
    st = gpu.blocked_encode_stream(img, True)
    ok = np.zeros((8, 8), dtype=np.uint32)
    for args, stride, code in (((0, 0, 0, 8), 8, "InvalidParameter"), ((0, 0, 8, 0), 8, "InvalidParameter"), ((0, 0, 8, 8), 7, "InvalidParameter"), ((60, 0, 8, 8), 8, "OutOfBounds"),
                               ((0, 64, 1, 1), 8, "OutOfBounds"), ((1 << 63, 0, 1 << 63, 1), 1 << 63, "OutOfBounds")):
        assert gpu.lib.limg_hip_blocked_decode_stream_window(gpu.ctx, st.ctypes.data, st.size, *args, ok.ctypes.data, stride) == ERRORS[code], args
    assert gpu.lib.limg_hip_blocked_decode_stream_window(gpu.ctx, None, st.size, 0, 0, 8, 8, ok.ctypes.data, 8) == ERRORS["ArgumentNull"]
    assert gpu.lib.limg_hip_blocked_decode_stream_window_device(gpu.ctx, None, st.size, 64, 64, 0, 0, 8, 8, ok.ctypes.data, 8, None) == ERRORS["ArgumentNull"]
    gpu.check()


def test_full_size_on_the_device(gpu):
    """8192^2 photo-noise and 4096^2 gradient: every window equals that slice of the plane path's pDecoded, on the device."""
    import torch
    for kind, n in (("photo_noise", 8192), ("random_gradient", 4096)):
        img = gpu.synth_device(kind, n, n, seed=1)
        planes = gpu.alloc_blocked_planes_device(n, n)
        gpu.blocked_encode3d_device(img, True, planes)
        torch.cuda.synchronize()
        st, nbytes = gpu.blocked_encode_stream_device(img, True)
        want = planes["pDecoded"]
        for i, win in enumerate(FULL_SIZE_WINDOWS(n)):
            device_window(gpu.blocked_decode_stream_window_device, st, nbytes, n, n, want, win, unaligned=bool(i & 1))
        gpu.check()
        del planes, st, img, want
        torch.cuda.empty_cache()


L.product_twins(globals())
