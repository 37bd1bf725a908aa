"""What the batched window decode tests of both stream versions share: many jobs laid out as disjoint slices of ONE sentinel-filled flat device tensor (the sentinel
discipline of tests/window_cases.py, for a whole job list at once), the expected tensor built from the crops, and the argument-error list of the batched entries."""
import ctypes as C

import numpy as np

import limg_amd
from window_cases import ERRORS, SENTINEL


class Batch:
    """add() jobs, then tensors(): (flat, expected).  A job's slice starts 16-byte aligned with a stride that is a multiple of 4 (so windows with x % 4 == 0 take the
    16-byte stores) or, unaligned, 4 bytes off a 16-byte boundary with an odd stride (every piece leaves as dword stores) -- the two placements of
    window_cases.device_window.  Between and around the slices, and in every row's stride slack, the sentinel must survive."""

    def __init__(self):
        self.jobs, self.off = [], 8

    def add(self, dstream, nbytes, W, H, want, win, unaligned):
        x, y, w, h = win
        stride = (w + 5) | 1 if unaligned else (w + 8) // 4 * 4
        start = (self.off + 3) // 4 * 4 + 4 + (1 if unaligned else 0)
        self.off = start + h * stride + 3
        self.jobs.append(dict(stream=dstream, nbytes=nbytes, W=W, H=H, want=want, win=win, stride=stride, start=start))
        return len(self.jobs) - 1

    def tensors(self):
        import torch
        n = self.off + 8
        flat = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")
        assert flat.data_ptr() % 16 == 0
        if all(isinstance(j["want"], np.ndarray) for j in self.jobs):
            exp = np.full(n, SENTINEL, dtype=np.uint32)
            for j in self.jobs:
                x, y, w, h = j["win"]
                exp[j["start"]:j["start"] + h * j["stride"]].reshape(h, j["stride"])[:, :w] = j["want"][y:y + h, x:x + w]
            exp = torch.from_numpy(exp.view(np.int32)).cuda()
        else:
            exp = torch.full_like(flat, SENTINEL)
            for j in self.jobs:
                x, y, w, h = j["win"]
                exp[j["start"]:j["start"] + h * j["stride"]].view(h, j["stride"])[:, :w] = j["want"][y:y + h, x:x + w]
        return flat, exp

    def args(self, flat, which=None):
        """the job tuples of LimgHip.*decode_stream_windows_device, writing into `flat`"""
        return [(j["stream"], j["nbytes"], j["W"], j["H"], *j["win"], flat[j["start"]:], j["stride"]) for j in (self.jobs if which is None else [self.jobs[i] for i in which])]

    def slice_of(self, t, i):
        """job i's window in tensor `t` (a flat tensor of this layout) as numpy uint32 (h, w)"""
        j = self.jobs[i]
        x, y, w, h = j["win"]
        return t[j["start"]:j["start"] + h * j["stride"]].view(h, j["stride"])[:, :w].cpu().numpy().view(np.uint32)


def run_and_compare(gpu, batched, single, batch, status_zero=True):
    """One batched call over the whole layout: the tensor equals the expected one, pJobStatus is all 0, and the same jobs issued one by one through the single-window
    entry give the identical tensor.  Returns the batched tensor."""
    import torch
    flat, exp = batch.tensors()
    status = torch.full((len(batch.jobs),), 77, dtype=torch.int32, device="cuda")
    batched(batch.args(flat), status=status)
    torch.cuda.synchronize()
    bad = torch.nonzero(flat != exp)[:6].ravel().tolist()
    assert not bad, (bad, [(i, j["win"], j["start"], j["stride"]) for i, j in enumerate(batch.jobs) if any(j["start"] - 8 <= b <= j["start"] + j["win"][3] * j["stride"] + 8 for b in bad)][:4])
    if status_zero:
        assert not bool(status.any()), status.cpu().tolist()
    one_by_one = torch.full_like(flat, SENTINEL)
    for a in batch.args(one_by_one):
        single(*a[:8], out=a[8], out_stride=a[9])
    torch.cuda.synchronize()
    assert torch.equal(one_by_one, flat)
    gpu.check()
    return flat


def device_stream(st, pad=64):
    """a host stream in device memory, 16-byte aligned, with zeroed slack behind it"""
    import torch
    d = torch.zeros(st.size + pad, dtype=torch.uint8, device="cuda")
    d[:st.size] = torch.from_numpy(np.ascontiguousarray(st)).cuda()
    assert d.data_ptr() % 16 == 0
    return d


def host_windows(decode, stream, want, wins):
    """The host form: every window into the middle of a sentinel-filled array of its own, with a stride larger than the width, in ONE call."""
    bufs = [np.full((h + 3, w + 7), SENTINEL, dtype=np.uint32) for x, y, w, h in wins]
    got = decode(stream, wins, outs=[b[1:1 + h, 2:2 + w] for b, (x, y, w, h) in zip(bufs, wins)])
    assert len(got) == len(wins)
    for b, (x, y, w, h) in zip(bufs, wins):
        exp = np.full_like(b, SENTINEL)
        exp[1:1 + h, 2:2 + w] = want[y:y + h, x:x + w]
        assert np.array_equal(b, exp), ((x, y, w, h), np.argwhere(b != exp)[:6].tolist())


def host_windows_refused(decode, stream, wins):
    """a stream that is refused for one window: the call raises and EVERY output is untouched"""
    import pytest
    bufs = [np.full((h, w + 3), SENTINEL, dtype=np.uint32) for x, y, w, h in wins]
    with pytest.raises(limg_amd.LimgHipError):
        decode(stream, wins, outs=[b[:, :w] for b, (x, y, w, h) in zip(bufs, wins)])
        pytest.fail("accepted")
    assert all((b == SENTINEL).all() for b in bufs)


def _name(r):
    return {v: k for k, v in ERRORS.items()}.get(r, r)


def argument_errors(gpu, entry, dstream, nbytes, W, H):
    """count == 0 and NULL jobs; job 2 of 4 bad in each way the single-window entry rejects: the right code comes back, and nothing was enqueued -- all four outputs
    still hold the sentinel.  `entry`: the C symbol's name; dstream: a good stream of a W x H image (W, H >= 16)."""
    import torch
    fn = getattr(gpu.lib, entry)
    s = gpu._stream()
    outs = [torch.full((8, 12), SENTINEL, dtype=torch.int32, device="cuda") for _ in range(4)]

    def table(bad=None):
        t = (limg_amd.WindowJob * 4)()
        for i in range(4):
            t[i] = limg_amd.WindowJob(dstream.data_ptr(), nbytes, W, H, limg_amd.Window(8 * i, 0, 8, 8, outs[i].data_ptr(), 12))
        if bad:
            bad(t[2])
        return t

    def setw(**kw):
        def f(j):
            for k, v in kw.items():
                setattr(j.window, k, v)
        return f

    assert _name(fn(gpu.ctx, table(), 0, None, s)) == "InvalidParameter"
    assert _name(fn(gpu.ctx, None, 4, None, s)) == "ArgumentNull"
    assert _name(fn(None, table(), 4, None, s)) == "ArgumentNull"
    cases = [
        ("zero width", setw(width=0), "InvalidParameter"),
        ("zero height", setw(height=0), "InvalidParameter"),
        ("stride < width", setw(outStridePixels=7), "InvalidParameter"),
        ("out of bounds", setw(x0=W - 4), "OutOfBounds"),
        ("below the image", setw(y0=H), "OutOfBounds"),
        ("overflow", setw(x0=1 << 63, width=1 << 63, outStridePixels=1 << 63), "OutOfBounds"),
        ("pOut misaligned by 2", setw(pOut=outs[2].data_ptr() + 2), "InvalidParameter"),
        ("pStream misaligned", lambda j: setattr(j, "pStream", dstream.data_ptr() + 4), "InvalidParameter"),
        ("NULL pOut", setw(pOut=None), "ArgumentNull"),
        ("NULL pStream", lambda j: setattr(j, "pStream", None), "ArgumentNull"),
        ("short stream", lambda j: setattr(j, "streamBytes", 32), "InvalidParameter"),
    ]
    for what, bad, code in cases:
        assert _name(fn(gpu.ctx, table(bad), 4, None, s)) == code, what
        torch.cuda.synchronize()
        assert all(bool((o == SENTINEL).all()) for o in outs), what
    gpu.check()
    assert fn(gpu.ctx, table(), 4, None, s) == 0  # the context is usable afterwards, and the good list decodes
    torch.cuda.synchronize()
    gpu.check()
    assert all(bool((o[:, :8] != SENTINEL).any()) and bool((o[:, 8:] == SENTINEL).all()) for o in outs)
    assert C.sizeof(limg_amd.Window) == 6 * C.sizeof(C.c_size_t) and C.sizeof(limg_amd.WindowJob) == 10 * C.sizeof(C.c_size_t)
