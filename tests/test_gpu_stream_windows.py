"""Batched window decode of the version 1 stream (limg_hip_decode_stream_windows*): job i of a call writes exactly what the single-window entry writes for the same
arguments -- the crop of the oracle's pDecoded -- and nothing else; a refused job never changes what another writes; every job is checked on the host before anything is
enqueued (tests/window_batch.py, tests/window_cases.py)."""
import numpy as np
import pytest

import lib_axis as L
import limg_amd
from oracle import stream as S
from test_gpu_stream import _cases
from window_batch import Batch, argument_errors, device_stream, host_windows, host_windows_refused, run_and_compare
from window_cases import SENTINEL, windows

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
    """(name, img, alpha, kw, pDecoded) of every image of test_gpu_stream._cases: computed once, shared, never changed"""
    if "cases" not in _REF:
        _REF["cases"] = [(name, img, alpha, kw, oracle.encode3d(img, alpha, **kw)["pDecoded"]) for name, img, alpha, kw in _cases(oracle)]
    return _REF["cases"]


def _pn64(oracle, gpu, seed=3):
    img = oracle.photo_noise(64, 64, seed)
    st = gpu.encode_stream(img, True)
    return st, gpu.decode_stream(st)


def test_mixed_batch(gpu, oracle):
    """every window of windows(W, H) of every image -- 3 and 4 channels, ragged sizes, more than 64 blocks per row -- in ONE call"""
    batch = Batch()
    for name, img, alpha, kw, want in _ref(oracle):
        H, W = img.shape
        st = gpu.encode_stream(img, alpha, **kw)
        d = device_stream(st)
        for win in windows(W, H):
            batch.add(d, st.size, W, H, want, win, unaligned=bool(len(batch.jobs) & 1))
    assert any(j["W"] == 2400 and j["win"][2] == 2400 for j in batch.jobs)  # several units per block row
    assert len({(j["W"], j["H"]) for j in batch.jobs}) >= 10 and len(batch.jobs) > 120
    run_and_compare(gpu, gpu.decode_stream_windows_device, gpu.decode_stream_window_device, batch)


def test_many_tiny_jobs(gpu, oracle):
    """300 jobs on one 256 x 64 stream: more jobs than waves in a launch's first workgroups, so the unit-to-job search crosses many boundaries"""
    import torch
    img = oracle.photo_noise(256, 64, 3)
    want = oracle.encode3d(img, True)["pDecoded"]
    st = gpu.encode_stream(img, True)
    d = device_stream(st)
    rng = np.random.RandomState(5)
    batch = Batch()
    for i in range(300):
        if i % 3 == 0:
            win = (int(rng.randint(0, 256)), int(rng.randint(0, 64)), 1, 1)
        elif i % 3 == 1:
            x = int(rng.randint(0, 256))
            win = (x, int(rng.randint(0, 64)), int(rng.randint(1, 257 - x)), 1)
        else:
            x, y = int(rng.randint(0, 256)), int(rng.randint(0, 64))
            win = (x, y, int(rng.randint(1, min(40, 256 - x) + 1)), int(rng.randint(1, min(20, 64 - y) + 1)))
        batch.add(d, st.size, 256, 64, want, win, unaligned=bool(i & 1))
    run_and_compare(gpu, gpu.decode_stream_windows_device, gpu.decode_stream_window_device, batch)
    # count == 1 equals the single-window entry
    for unaligned in (False, True):
        one = Batch()
        one.add(d, st.size, 256, 64, want, (13, 5, 100, 41), unaligned)
        run_and_compare(gpu, gpu.decode_stream_windows_device, gpu.decode_stream_window_device, one)
    out, = gpu.decode_stream_windows_device([(d, st.size, 256, 64, 8, 8, 32, 16, None, None)])  # out=None allocates
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want[8:24, 8:40])


def test_two_calls_back_to_back(gpu, oracle):
    """a second call issued before the first has run does not disturb the first call's job table"""
    import torch
    img = oracle.photo_noise(256, 64, 3)
    want = oracle.encode3d(img, True)["pDecoded"]
    st = gpu.encode_stream(img, True)
    d = device_stream(st)
    first, second = Batch(), Batch()
    for i, win in enumerate(windows(256, 64)):
        first.add(d, st.size, 256, 64, want, win, unaligned=bool(i & 1))
    for i, win in enumerate(windows(256, 64, seed=2)[::-1] + [(3, 3, 250, 60)]):
        second.add(d, st.size, 256, 64, want, win, unaligned=not (i & 1))
    (f1, e1), (f2, e2) = first.tensors(), second.tensors()
    a1, a2 = first.args(f1), second.args(f2)
    torch.cuda.synchronize()
    for _ in range(3):  # (more calls in flight than the ring has slots)
        gpu.decode_stream_windows_device(a1)
        gpu.decode_stream_windows_device(a2)
    torch.cuda.synchronize()
    assert torch.equal(f1, e1) and torch.equal(f2, e2)
    gpu.check()


def test_refusals(gpu, oracle):
    import torch
    st, want = _pn64(oracle, gpu)
    st2, want2 = _pn64(oracle, gpu, seed=9)
    table = len(S.parse(st)[1])
    win = (10, 9, 40, 30)  # blocks 1 .. 6 of block rows 1 .. 4
    evil = st.copy()
    evil[64:64 + 56 * table].view(S.BLOCK)["payloadWord"][2 * 8 + 3] = 0x7FFFFFF0  # block (3, 2): inside the window
    outs = [torch.full((30, 43), SENTINEL, dtype=torch.int32, device="cuda") for _ in range(3)]
    status = torch.full((3,), 77, dtype=torch.int32, device="cuda")
    streams = [device_stream(s) for s in (st, evil, st2)]
    gpu.decode_stream_windows_device([(d, st.size, 64, 64, *win, o, 43) for d, o in zip(streams, outs)], status=status)
    torch.cuda.synchronize()
    with pytest.raises(limg_amd.LimgHipError):
        gpu.check()
    gpu.check()  # reported once
    got = [o.cpu().numpy().view(np.uint32) for o in outs]
    assert all((g[:, 40:] == SENTINEL).all() for g in got)
    assert np.array_equal(got[0][:, :40], want[9:39, 10:50]) and np.array_equal(got[2][:, :40], want2[9:39, 10:50])
    # block row 2 (image rows 16 .. 23) is the refused group: it stores nothing, the job's other groups are stored
    assert (got[1][7:15, :40] == SENTINEL).all() and np.array_equal(got[1][:7, :40], want[9:16, 10:50]) and np.array_equal(got[1][15:, :40], want[24:39, 10:50])
    s = status.cpu().tolist()
    assert s[0] == 0 and s[2] == 0 and s[1] == 2, s
    # a job with a bad magic writes nothing (bit 0); a bad entry OUTSIDE a job's window does not concern it; a version 2 stream is a header mismatch
    bad = st.copy(); bad[0] ^= 0xFF
    outside = st.copy()
    outside[64:64 + 56 * table].view(S.BLOCK)["payloadWord"][7 * 8 + 7] = 0x7FFFFFF0
    v2 = gpu.blocked_encode_stream(oracle.photo_noise(64, 64, 3), True)
    streams = [device_stream(s, pad=64 * 56) for s in (bad, outside, v2)]
    outs = [torch.full((30, 43), SENTINEL, dtype=torch.int32, device="cuda") for _ in range(3)]
    gpu.decode_stream_windows_device([(d, st.size, 64, 64, *win, o, 43) for d, o in zip(streams, outs)], status=status)
    torch.cuda.synchronize()
    with pytest.raises(limg_amd.LimgHipError):
        gpu.check()
    gpu.check()
    got = [o.cpu().numpy().view(np.uint32) for o in outs]
    assert (got[0] == SENTINEL).all() and (got[2] == SENTINEL).all()
    assert np.array_equal(got[1][:, :40], want[9:39, 10:50]) and (got[1][:, 40:] == SENTINEL).all()
    s = status.cpu().tolist()
    assert s[0] & 1 and s[1] == 0 and s[2] & 1, s
    # every call overwrites the status words: a good list after a refused one
    gpu.decode_stream_windows_device([(streams[1], st.size, 64, 64, *win, outs[0], 43)] * 3, status=status)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0, 0, 0]
    gpu.check()


def test_argument_errors(gpu, oracle):
    st, _ = _pn64(oracle, gpu)
    argument_errors(gpu, "limg_hip_decode_stream_windows_device", device_stream(st), st.size, 64, 64)
    # the table's extent against streamBytes, per job (the single-window entry's last check)
    import torch
    d = device_stream(st)
    out = torch.full((8, 8), SENTINEL, dtype=torch.int32, device="cuda")
    t = (limg_amd.WindowJob * 2)(limg_amd.WindowJob(d.data_ptr(), st.size, 64, 64, limg_amd.Window(0, 0, 8, 8, out.data_ptr(), 8)),
                                 limg_amd.WindowJob(d.data_ptr(), 64 + 56 * 64 - 1, 64, 64, limg_amd.Window(0, 0, 8, 8, out.data_ptr(), 8)))
    assert gpu.lib.limg_hip_decode_stream_windows_device(gpu.ctx, t, 2, None, gpu._stream()) == 103
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    # the host form's own: NULL windows, count == 0, one bad window of three
    ok = np.full((8, 9), SENTINEL, dtype=np.uint32)
    W = limg_amd.Window
    fn = gpu.lib.limg_hip_decode_stream_windows
    good = [W(0, 0, 8, 8, ok.ctypes.data, 9), W(8, 8, 8, 8, ok.ctypes.data, 9)]
    assert fn(gpu.ctx, st.ctypes.data, st.size, None, 3) == 102 and fn(gpu.ctx, None, st.size, (W * 2)(*good), 2) == 102
    assert fn(gpu.ctx, st.ctypes.data, st.size, (W * 2)(*good), 0) == 101
    for bad, code in ((W(0, 0, 0, 8, ok.ctypes.data, 9), 101), (W(0, 0, 8, 8, ok.ctypes.data, 7), 101), (W(60, 0, 8, 8, ok.ctypes.data, 9), 103),
                      (W(1 << 63, 0, 1 << 63, 1, ok.ctypes.data, 1 << 63), 103), (W(0, 0, 8, 8, None, 9), 102)):
        assert fn(gpu.ctx, st.ctypes.data, st.size, (W * 3)(good[0], good[1], bad), 3) == code, (bad.x0, bad.width, code)
        assert (ok == SENTINEL).all()
    gpu.check()


def test_host_form(gpu, oracle):
    for name, img, alpha, kw, want in _ref(oracle):
        H, W = img.shape
        st = gpu.encode_stream(img, alpha, **kw)
        host_windows(gpu.decode_stream_windows, st, want, windows(W, H))
    got = gpu.decode_stream_windows(st, [(0, 0, W, H), (5, 3, 9, 2)])  # outs=None allocates
    assert np.array_equal(got[0], want) and np.array_equal(got[1], want[3:5, 5:14])
    # a stream that is refused for ONE window leaves every output untouched
    st, _ = _pn64(oracle, gpu)
    evil = st.copy()
    evil[64:64 + 56 * 64].view(S.BLOCK)["payloadWord"][2 * 8 + 3] = 0x7FFFFFF0
    host_windows_refused(gpu.decode_stream_windows, evil, [(0, 0, 8, 8), (10, 9, 40, 30), (56, 56, 8, 8)])
    gpu.check()
    bad = st.copy(); bad[0] ^= 0xFF
    host_windows_refused(gpu.decode_stream_windows, bad, [(0, 0, 8, 8)])
    host_windows_refused(gpu.decode_stream_windows, st[:st.size - 8], [(0, 0, 8, 8)])
    gpu.check()


def test_mid_size_on_the_device(gpu):
    """2048^2 photo-noise synthesised on the device, 64 seeded windows of at most 256^2 in one call, against the plane path's pDecoded"""
    import torch
    n = 2048
    img = gpu.synth_device("photo_noise", n, n, seed=1)
    planes = gpu.alloc_planes_device(n, n)
    gpu.encode3d_device(img, True, planes)
    st, nbytes = gpu.encode_stream_device(img, True)
    rng = np.random.RandomState(11)
    batch = Batch()
    for i in range(64):
        w, h = int(rng.randint(1, 257)), int(rng.randint(1, 257))
        x, y = int(rng.randint(0, n - w + 1)), int(rng.randint(0, n - h + 1))
        if i % 4 == 0:
            x, y, w, h = x // 8 * 8, y // 8 * 8, 256, 256  # block-aligned
            x, y = min(x, n - 256), min(y, n - 256)
        batch.add(st, nbytes, n, n, planes["pDecoded"], (x, y, w, h), unaligned=bool(i & 1))
    run_and_compare(gpu, gpu.decode_stream_windows_device, gpu.decode_stream_window_device, batch)
    del planes, st, img, batch
    torch.cuda.empty_cache()


L.product_twins(globals())
