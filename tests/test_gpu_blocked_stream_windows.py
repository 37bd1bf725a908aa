"""Batched window decode of the version 2 stream (limg_hip_blocked_decode_stream_windows*): job i of a call writes exactly what the single-window entry writes for the
same arguments -- the crop of the oracle's limg_blocked_encode3d_test pDecoded -- and nothing else; jobs that name the same stream form a group whose rectangle table is
scanned once: a malformed table refuses every job of its group, a clash the job in whose window it lies, and no other job is changed (tests/window_batch.py)."""
import numpy as np
import pytest

import lib_axis as L
import limg_amd
from blocked_stream_ref import small_cases
from test_gpu_blocked_stream import _encode
from test_gpu_blocked_stream_window import _inside, _mutations
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
    """(name, img, alpha, kw, pDecoded) of every image of blocked_stream_ref.small_cases: computed once, shared, never changed"""
    if "cases" not in _REF:
        _REF["cases"] = [(name, img, alpha, kw, oracle.blocked_encode3d(img, alpha, **kw)["pDecoded"]) for name, img, alpha, kw in small_cases(oracle)]
    return _REF["cases"]


def _streams(gpu, oracle):
    """per image: (name, stream bytes, W, H, pDecoded, windows(W, H) + the _inside window)"""
    out, cut = [], 0
    for name, img, alpha, kw, want in _ref(oracle):
        st = _encode(gpu, img, alpha, kw)
        H, W = img.shape
        wins = windows(W, H)
        inside = _inside(gpu.blocked_regions(), W, H)
        if inside:
            wins.append(inside)
            cut += 1
        out.append((name, st, W, H, want, wins))
    assert cut >= 3
    return out


def test_mixed_batch(gpu, oracle):
    """every window of every image in ONE call: several jobs per stream, so groups form, and several streams"""
    batch = Batch()
    for name, st, W, H, want, wins in _streams(gpu, oracle):
        d = device_stream(st)
        for win in wins:
            batch.add(d, st.size, W, H, want, win, unaligned=bool(len(batch.jobs) & 1))
    assert len({j["stream"].data_ptr() for j in batch.jobs}) >= 20 and len(batch.jobs) > 250
    # the jobs of a stream are not neighbours in the list: groups are formed by the stream, not by the order
    order = np.random.RandomState(3).permutation(len(batch.jobs))
    batch.jobs = [batch.jobs[i] for i in order]
    run_and_compare(gpu, gpu.blocked_decode_stream_windows_device, gpu.blocked_decode_stream_window_device, batch)


def test_two_calls_back_to_back(gpu, oracle):
    """a second call issued before the first has run disturbs neither the first call's job table nor its map and verdict words"""
    import torch
    name, st, W, H, want, wins = _streams(gpu, oracle)[1]  # the 256 x 128 gradient
    d = device_stream(st)
    first, second = Batch(), Batch()
    for i, win in enumerate(wins):
        first.add(d, st.size, W, H, want, win, unaligned=bool(i & 1))
    for i, win in enumerate(windows(W, H, seed=2)[::-1] + [(3, 3, W - 6, H - 4)]):
        second.add(d, st.size, W, H, want, win, unaligned=not (i & 1))
    (f1, e1), (f2, e2) = first.tensors(), second.tensors()
    a1, a2 = first.args(f1), second.args(f2)
    torch.cuda.synchronize()
    for _ in range(3):  # (more calls in flight than the ring has slots)
        gpu.blocked_decode_stream_windows_device(a1)
        gpu.blocked_decode_stream_windows_device(a2)
    torch.cuda.synchronize()
    assert torch.equal(f1, e1) and torch.equal(f2, e2)
    gpu.check()


def test_argument_errors(gpu, oracle):
    st = gpu.blocked_encode_stream(oracle.photo_noise(64, 64, 3), True)
    argument_errors(gpu, "limg_hip_blocked_decode_stream_windows_device", device_stream(st), st.size, 64, 64)
    ok = np.full((8, 9), SENTINEL, dtype=np.uint32)
    W = limg_amd.Window
    fn = gpu.lib.limg_hip_blocked_decode_stream_windows
    good = [W(0, 0, 8, 8, ok.ctypes.data, 9), W(8, 8, 8, 8, ok.ctypes.data, 9)]
    assert fn(gpu.ctx, st.ctypes.data, st.size, None, 3) == 102 and fn(gpu.ctx, None, st.size, (W * 2)(*good), 2) == 102
    assert fn(gpu.ctx, st.ctypes.data, st.size, (W * 2)(*good), 0) == 101
    for bad, code in ((W(0, 0, 0, 8, ok.ctypes.data, 9), 101), (W(0, 0, 8, 8, ok.ctypes.data, 7), 101), (W(60, 0, 8, 8, ok.ctypes.data, 9), 103),
                      (W(1 << 63, 0, 1 << 63, 1, ok.ctypes.data, 1 << 63), 103), (W(0, 0, 8, 8, None, 9), 102)):
        assert fn(gpu.ctx, st.ctypes.data, st.size, (W * 3)(good[0], good[1], bad), 3) == code, (bad.x0, bad.width, code)
        assert (ok == SENTINEL).all()
    gpu.check()


def test_host_form(gpu, oracle):
    for name, st, W, H, want, wins in _streams(gpu, oracle):
        host_windows(gpu.blocked_decode_stream_windows, st, want, wins)
    got = gpu.blocked_decode_stream_windows(st, [(0, 0, W, H)])  # outs=None allocates
    assert np.array_equal(got[0], want)
    # a stream that is refused for ONE window leaves every output untouched
    img, good, win, cases = _mutations(oracle, gpu)
    for name in ("window block claimed twice", "payloadWord past the end", "wrong magic"):
        host_windows_refused(gpu.blocked_decode_stream_windows, cases[name], [(0, 0, 1, 1), win, (0, 0, 64, 48)])
        gpu.check()
    with pytest.raises(limg_amd.LimgHipError):
        gpu.decode_stream_windows(good, [win])  # version 2 bytes given to the version 1 entry


def test_group_semantics(gpu, oracle):
    """On the 64 x 48 gradient of _mutations: a clash concerns the job in whose window it lies, a malformed table every job of its stream, and no other stream's jobs."""
    import torch
    from oracle import blocked_stream as B
    img, good, win, cases = _mutations(oracle, gpu)
    want = oracle.blocked_encode3d(img, True)["pDecoded"]
    table = B.parse(good)[1]
    big = table[int(np.argmax(table["rx"].astype(int) * table["ry"]))]
    other_win = (int(big["ox"]) * 8 + 1, int(big["oy"]) * 8 + 1, 5, 6)  # inside block (ox, oy) of the largest rectangle: the block claimed twice is (ox + 1, oy + 1)
    assert win[0] // 8 == big["ox"] and (win[0] + win[2] - 1) // 8 >= big["ox"] + 1 and (win[1] + win[3] - 1) // 8 >= big["oy"] + 1
    intact = device_stream(good)

    def run(evil, jobs_of_evil):
        d = device_stream(evil, pad=64 * 64 + 64)
        wins = jobs_of_evil + [win]
        streams = [d] * len(jobs_of_evil) + [intact]
        outs = [torch.full((w[3], w[2] + 3), SENTINEL, dtype=torch.int32, device="cuda") for w in wins]
        status = torch.full((len(wins),), 77, dtype=torch.int32, device="cuda")
        gpu.blocked_decode_stream_windows_device([(s, evil.size if s is d else good.size, 64, 48, *w, o, w[2] + 3) for s, w, o in zip(streams, wins, outs)], status=status)
        torch.cuda.synchronize()
        with pytest.raises(limg_amd.LimgHipError):
            gpu.check()
        gpu.check()  # reported once
        got = [o.cpu().numpy().view(np.uint32) for o in outs]
        assert all((g[:, w[2]:] == SENTINEL).all() for g, w in zip(got, wins))
        decoded = [bool(np.array_equal(g[:, :w[2]], want[w[1]:w[1] + w[3], w[0]:w[0] + w[2]])) for g, w in zip(got, wins)]
        untouched = [bool((g == SENTINEL).all()) for g in got]
        return decoded, untouched, status.cpu().tolist()

    # one block claimed twice inside window A, outside window B of the same stream: A is refused and writes nothing, B and the intact stream's job are decoded
    decoded, untouched, status = run(cases["window block claimed twice"], [win, other_win])
    assert untouched[0] and decoded[1] and decoded[2], (decoded, untouched)
    assert status[0] & 2 and status[1] == 0 and status[2] == 0, status
    # a rectangle outside the block grid, a payloadWord past the end: every job of that stream is refused, the other stream's job is decoded
    for name in ("rect outside", "payloadWord past the end"):
        decoded, untouched, status = run(cases[name], [win, other_win, (0, 0, 64, 48)])
        assert untouched[:3] == [True] * 3 and decoded[3], (name, decoded, untouched)
        assert all(s & 2 for s in status[:3]) and status[3] == 0, (name, status)
    # a header that does not match: bit 0 for every job of the stream
    decoded, untouched, status = run(cases["wrong magic"], [win, other_win])
    assert untouched[:2] == [True] * 2 and decoded[2] and all(s & 1 for s in status[:2]) and status[2] == 0, (decoded, untouched, status)
    decoded, untouched, status = run(cases["version 1 bytes"], [win])
    assert untouched[0] and decoded[1] and status[0] & 1 and status[1] == 0, (decoded, untouched, status)


def test_window_that_cuts_a_rectangle(gpu, oracle):
    """The 256 x 128 gradient: the three windows of test_gpu_blocked_stream_window.test_window_that_cuts_a_rectangle plus the whole image, in one call."""
    img = oracle.random_gradient(256, 128, 5, True)
    want = oracle.blocked_encode3d(img, True)
    st = gpu.blocked_encode_stream(img, True)
    win = _inside(gpu.blocked_regions(), 256, 128)
    assert win is not None and win == _inside(want["regions"], 256, 128)
    d = device_stream(st)
    for flip in (False, True):
        batch = Batch()
        for i, w in enumerate([win, (win[0] + 8, win[1] + 8, 1, 1), (win[0], win[1], win[2], 1), (0, 0, 256, 128)]):
            batch.add(d, st.size, 256, 128, want["pDecoded"], w, unaligned=bool(i & 1) != flip)
        run_and_compare(gpu, gpu.blocked_decode_stream_windows_device, gpu.blocked_decode_stream_window_device, batch)


L.product_twins(globals())
