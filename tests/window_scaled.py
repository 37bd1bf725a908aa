"""What the reduced-scale window decode tests of both stream versions share (limg_hip_*decode_stream_windows_scaled*): the numpy statement of the contract's box
reduction, the job layouts of tests/window_batch.py and tests/window_tensor.py with a level per job, and the test bodies that do not depend on the stream version.
A stream is (device stream, nbytes, W, H, pyramid); pyramid[L] is the ORACLE's decoded image reduced to level L in numpy -- expected pixels never come from the
library's own decode.  Everything is compared on bit patterns, in sentinel-filled outputs."""
import ctypes as C

import numpy as np

import limg_amd
import window_tensor as T
from window_batch import Batch
from window_cases import ERRORS, SENTINEL, windows

LEVELS = (0, 1, 2, 3)
MODES = ["rgba"] + T.FORMATS  # how the pixels leave: packed RGBA8 or (dtype, planes, constants)


def mode_id(m):
    return m if m == "rgba" else "-".join(str(v) for v in m)


def reduce(img, L):
    """(H, W) uint32 -> (H >> L, W >> L) uint32 by the contract's formula: per byte the sum of the k x k box plus k * k >> 1, shifted right by 2 L; trailing rows and
    columns that do not fill a box are dropped"""
    k = 1 << L
    RY, RX = img.shape[0] >> L, img.shape[1] >> L
    if RX == 0 or RY == 0:
        return np.zeros((RY, RX), dtype=np.uint32)
    b = np.ascontiguousarray(img[:RY * k, :RX * k]).view(np.uint8).reshape(RY, k, RX, k, 4).astype(np.uint32)
    q = (b.sum(axis=(1, 3), dtype=np.uint32) + np.uint32((k * k) >> 1)) >> np.uint32(2 * L)
    return np.ascontiguousarray(q.astype(np.uint8)).view(np.uint32).reshape(RY, RX)


def pyramid(img):
    return [reduce(img, L) for L in LEVELS]


def entry(gpu, blocked, tensor, host=False):
    """the LimgHip method of the version / output kind / pointer kind"""
    return getattr(gpu, ("blocked_" if blocked else "") + "decode_stream_windows_scaled" + ("_tensor" if tensor else "") + ("" if host else "_device"))


def plain_entry(gpu, blocked, tensor):
    """the existing batched entry (full scale only)"""
    return getattr(gpu, ("blocked_" if blocked else "") + "decode_stream_windows" + ("_tensor" if tensor else "") + "_device")


class ScaledBatch(Batch):
    """window_batch.Batch whose jobs carry a level: a job's window is in that level's coordinates and its expectation the crop of pyramid[level]"""

    def add(self, dstream, nbytes, W, H, pyr, level, win, unaligned):
        k = super().add(dstream, nbytes, W, H, pyr[level], win, unaligned)
        self.jobs[k]["level"] = level
        return k

    def args(self, flat, which=None):
        return [(j["stream"], j["nbytes"], j["W"], j["H"], j["level"], *j["win"], flat[j["start"]:], j["stride"]) for j in (self.jobs if which is None else [self.jobs[i] for i in which])]

    def plain_args(self, flat):
        assert all(j["level"] == 0 for j in self.jobs)
        return super().args(flat)


class ScaledTensorBatch(T.TensorBatch):
    def add(self, dstream, nbytes, W, H, pyr, level, win, unaligned):
        k = super().add(dstream, nbytes, W, H, pyr[level], win, unaligned)
        self.jobs[k]["level"] = level
        return k

    def args(self, flat, which=None):
        return [(j["stream"], j["nbytes"], j["W"], j["H"], j["level"], *j["win"], flat[j["start"]:], j["row"], j["plane"]) for j in (self.jobs if which is None else [self.jobs[i] for i in which])]

    def plain_args(self, flat):
        assert all(j["level"] == 0 for j in self.jobs)
        return super().args(flat)


def new_batch(mode):
    return ScaledBatch() if mode == "rgba" else ScaledTensorBatch(*mode)


def fill(batch, streams, levels=LEVELS):
    """every window of windows(RX, RY) of every level of every image, aligned and misaligned placements alternating; a level whose image is empty is skipped"""
    for d, nbytes, W, H, pyr in streams:
        for L in levels:
            RX, RY = W >> L, H >> L
            if RX == 0 or RY == 0:
                continue
            for win in windows(RX, RY):
                batch.add(d, nbytes, W, H, pyr, L, win, unaligned=bool(len(batch.jobs) & 1))
    return batch


def run_rgba(gpu, call, batch, one_by_one=True):
    """one call over the whole layout: the buffer equals the expected one, sentinels included; pJobStatus is all 0; the same jobs one per call give the identical buffer"""
    import torch
    flat, exp = batch.tensors()
    status = torch.full((len(batch.jobs),), 77, dtype=torch.int32, device="cuda")
    call(batch.args(flat), status=status)
    torch.cuda.synchronize()
    bad = torch.nonzero(flat != exp)[:6].ravel().tolist()
    assert not bad, (bad, [(i, j["level"], j["win"], j["start"], j["stride"]) for i, j in enumerate(batch.jobs)
                           if any(j["start"] - 8 <= b <= j["start"] + j["win"][3] * j["stride"] + 8 for b in bad)][:4])
    assert not bool(status.any()), status.cpu().tolist()
    if one_by_one:
        again = torch.full_like(flat, SENTINEL)
        for a in batch.args(again):
            call([a])
        torch.cuda.synchronize()
        assert torch.equal(again, flat)
    gpu.check()
    return flat


def run(gpu, blocked, batch, mode, one_by_one=True):
    if mode == "rgba":
        return run_rgba(gpu, entry(gpu, blocked, False), batch, one_by_one)
    return T.run_and_compare(gpu, entry(gpu, blocked, True), batch, one_by_one)


def mixed_batch(gpu, blocked, streams, mode):
    """all levels of all images mixed in ONE call"""
    batch = fill(new_batch(mode), streams)
    assert {j["level"] for j in batch.jobs} == set(LEVELS)
    for L in LEVELS:  # both placements occur at every level
        assert len({bool(i & 1) for i, j in enumerate(batch.jobs) if j["level"] == L}) == 2
    run(gpu, blocked, batch, mode)


def level0_equals_existing(gpu, blocked, streams):
    """the same jobs through the scaled entry at level 0 and through the existing batched entry: identical buffers, RGBA and tensor"""
    import torch
    for mode in ("rgba", ("float32", 3, "A"), ("float16", 4, "B")):
        batch = fill(new_batch(mode), streams, levels=(0,))
        if mode == "rgba":
            a = run_rgba(gpu, entry(gpu, blocked, False), batch, one_by_one=False)
            b = torch.full_like(a, SENTINEL)
            plain_entry(gpu, blocked, False)(batch.plain_args(b))
        else:
            a = T.run_and_compare(gpu, entry(gpu, blocked, True), batch, one_by_one=False)
            b, flat = T.sentinel_tensor(tuple(a.shape), mode[0])
            plain_entry(gpu, blocked, True)(batch.plain_args(flat), T.fmt_of(*mode))
        torch.cuda.synchronize()
        assert torch.equal(a, b), mode
    gpu.check()


def tensor_equals_conversion_of_rgba(gpu, blocked, stream):
    """levels 1 to 3: the scaled tensor output is window_tensor.convert of the scaled RGBA output of the same jobs -- the rounding happens before the float step"""
    import torch
    d, nbytes, W, H, pyr = stream
    jobs = []
    for L in (1, 2, 3):
        RX, RY = W >> L, H >> L
        jobs += [(L, 0, 0, RX, RY), (L, 1, 1, RX - 2, RY - 1), (L, RX // 2, 0, RX - RX // 2, RY)]
    rgba = entry(gpu, blocked, False)([(d, nbytes, W, H, L, x, y, w, h, None, None) for L, x, y, w, h in jobs])
    torch.cuda.synchronize()
    rgba = [r.cpu().numpy().view(np.uint32) for r in rgba]
    for (L, x, y, w, h), r in zip(jobs, rgba):
        assert np.array_equal(r, pyr[L][y:y + h, x:x + w]), (L, x, y, w, h)
    for dtype, planes, consts in T.FORMATS:
        got = entry(gpu, blocked, True)([(d, nbytes, W, H, L, x, y, w, h, None, None, None) for L, x, y, w, h in jobs], T.fmt_of(dtype, planes, consts))
        torch.cuda.synchronize()
        for job, r, g in zip(jobs, rgba, got):
            assert np.array_equal(g.cpu().numpy().view(T.BITS[dtype]), T.convert(r, dtype, planes, consts).view(T.BITS[dtype])), (job, dtype, planes, consts)
    gpu.check()


def crops(gpu, blocked, streams, dtype, planes):
    """decode_crops_scaled_device: 24 crops of 20 x 12 out of three streams, levels cycling through 0 .. 3, into one contiguous tensor and into a caller's tensor with a
    sentinel slice behind it = the stacked numpy expectation"""
    import torch
    assert len(streams) == 3
    tb, tf = T._torch_bits(dtype)
    rng = np.random.RandomState(11)
    jobs, want = [], []
    for i in range(24):
        d, nbytes, W, H, pyr = streams[i % 3]
        L = i % 4
        RX, RY = W >> L, H >> L
        assert RX >= 20 and RY >= 12, (W, H, L)
        x, y = int(rng.randint(0, RX - 20 + 1)), int(rng.randint(0, RY - 12 + 1))
        if i % 8 < 4:
            x = x // 4 * 4
        jobs.append((d, nbytes, W, H, L, x, y))
        want.append(torch.from_numpy(T.convert(pyr[L][y:y + 12, x:x + 20], dtype, planes, "A")))
    scale, bias = T.CONSTANTS["A"]
    out = gpu.decode_crops_scaled_device(jobs, 12, 20, tf, scale[:planes], bias[:planes], planes=planes, blocked=blocked)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (24, planes, 12, 20) and out.is_contiguous() and out.dtype == tf
    assert torch.equal(out.cpu().view(tb), torch.stack(want).view(tb))
    bits, flat = T.sentinel_tensor((25, planes, 12, 20), dtype)
    assert gpu.decode_crops_scaled_device(jobs, 12, 20, tf, scale[:planes], bias[:planes], planes=planes, blocked=blocked, out=flat[:24]).data_ptr() == flat.data_ptr()
    torch.cuda.synchronize()
    assert torch.equal(bits[:24].cpu(), torch.stack(want).view(tb)) and bool((bits[24] == T.SENT[dtype]).all())
    gpu.check()


def back_to_back(gpu, blocked, stream):
    """six scaled calls issued without synchronising, RGBA and tensor alternating -- more than the ring's four slots: both layouts come out correct"""
    import torch
    first, second = fill(ScaledBatch(), [stream]), ScaledTensorBatch("float16", 4, "B")
    d, nbytes, W, H, pyr = stream
    for L in LEVELS[::-1]:
        for i, win in enumerate(windows(W >> L, H >> L, seed=2)):
            second.add(d, nbytes, W, H, pyr, L, win, unaligned=not (i & 1))
    (f1, e1), (b2, f2, e2) = first.tensors(), second.tensors()
    a1, a2, m2 = first.args(f1), second.args(f2), T.fmt_of("float16", 4, "B")
    torch.cuda.synchronize()
    for _ in range(3):
        entry(gpu, blocked, False)(a1)
        entry(gpu, blocked, True)(a2, m2)
    torch.cuda.synchronize()
    assert torch.equal(f1, e1) and torch.equal(b2, e2)
    gpu.check()


def _pyramid_windows(W, H):
    """(level, x, y, w, h): every level's whole image and one window of it with no edge on the image's"""
    wins = []
    for L in LEVELS:
        RX, RY = W >> L, H >> L
        wins += [(L, 0, 0, RX, RY), (L, 1, 1, max(1, RX - 3), max(1, RY - 2))]
    return wins


def host_forms(gpu, blocked, st, W, H, pyr):
    """all four levels of one stream in ONE call, each window into the middle of a sentinel array with slack: RGBA, then two tensor formats"""
    wins = _pyramid_windows(W, H)
    bufs = [np.full((h + 3, w + 7), SENTINEL, dtype=np.uint32) for L, x, y, w, h in wins]
    got = entry(gpu, blocked, False, host=True)(st, wins, outs=[b[1:1 + h, 2:2 + w] for b, (L, x, y, w, h) in zip(bufs, wins)])
    assert len(got) == len(wins)
    for b, (L, x, y, w, h) in zip(bufs, wins):
        exp = np.full_like(b, SENTINEL)
        exp[1:1 + h, 2:2 + w] = pyr[L][y:y + h, x:x + w]
        assert np.array_equal(b, exp), ((L, x, y, w, h), np.argwhere(b != exp)[:6].tolist())
    for dtype, planes, consts in (("float32", 3, "A"), ("float16", 4, "B")):
        bufs = [np.full((planes + 1, h + 3, w + 7), T.SENT[dtype], dtype=T.BITS[dtype]) for L, x, y, w, h in wins]
        entry(gpu, blocked, True, host=True)(st, wins, T.fmt_of(dtype, planes, consts),
                                            outs=[b.view(T.NP[dtype])[:planes, 1:1 + h, 2:2 + w] for b, (L, x, y, w, h) in zip(bufs, wins)])
        for b, (L, x, y, w, h) in zip(bufs, wins):
            exp = np.full_like(b, T.SENT[dtype])
            exp[:planes, 1:1 + h, 2:2 + w] = T.convert(pyr[L][y:y + h, x:x + w], dtype, planes, consts).view(T.BITS[dtype])
            assert np.array_equal(b, exp), ((L, x, y, w, h), dtype, np.argwhere(b != exp)[:6].tolist())
    got = entry(gpu, blocked, False, host=True)(st, [(2, 0, 0, W >> 2, H >> 2)])  # outs=None allocates
    assert np.array_equal(got[0], pyr[2])
    gpu.check()


def host_forms_refused(gpu, blocked, evil, wins):
    """a stream that is refused for one window: the call raises and EVERY output is untouched, RGBA and tensor"""
    import pytest
    bufs = [np.full((h, w + 3), SENTINEL, dtype=np.uint32) for L, x, y, w, h in wins]
    with pytest.raises(limg_amd.LimgHipError):
        entry(gpu, blocked, False, host=True)(evil, wins, outs=[b[:, :w] for b, (L, x, y, w, h) in zip(bufs, wins)])
        pytest.fail("accepted")
    assert all((b == SENTINEL).all() for b in bufs)
    gpu.check()
    bufs = [np.full((3, h, w + 3), T.SENT["float32"], dtype=np.int32) for L, x, y, w, h in wins]
    with pytest.raises(limg_amd.LimgHipError):
        entry(gpu, blocked, True, host=True)(evil, wins, T.fmt_of("float32", 3, "A"), outs=[b.view(np.float32)[:, :, :w] for b, (L, x, y, w, h) in zip(bufs, wins)])
        pytest.fail("accepted")
    assert all((b == T.SENT["float32"]).all() for b in bufs)
    gpu.check()


def _name(r):
    return {v: k for k, v in ERRORS.items()}.get(r, r)


def struct_sizes():
    z = C.sizeof(C.c_size_t)
    assert C.sizeof(limg_amd.ScaledWindow) == 7 * z and C.sizeof(limg_amd.ScaledWindowJob) == 11 * z
    assert C.sizeof(limg_amd.ScaledTensorWindow) == 8 * z and C.sizeof(limg_amd.ScaledTensorWindowJob) == 12 * z
    assert limg_amd.ScaledWindow.log2Scale.offset == 6 * z and limg_amd.ScaledTensorWindow.log2Scale.offset == 7 * z


def device_argument_errors(gpu, name, tensor, dstream, nbytes, W, H, dtiny, tiny_bytes):
    """`name`: the C symbol of a scaled device entry; dstream: a good stream of a W x H image (W, H >= 64); dtiny: a good stream of a 5 x 3 image.  NULL and count 0 in
    the documented order; job 2 of 4 bad in each way: the right code comes back and nothing was enqueued -- all four outputs still hold the sentinel; then a good list
    decodes."""
    import torch
    fn = getattr(gpu.lib, name)
    s = gpu._stream()
    f32 = T.fmt_of("float32", 3, "A")
    outs = [torch.full((3, 8, 12), SENTINEL, dtype=torch.int32, device="cuda") for _ in range(4)]  # (as int32 bit patterns: float32 planes or, plane 0, pixels)
    J, Wn = (limg_amd.ScaledTensorWindowJob, limg_amd.ScaledTensorWindow) if tensor else (limg_amd.ScaledWindowJob, limg_amd.ScaledWindow)

    def call(t, count, jobs_null=False, ctx_null=False, fmt=f32):
        extra = (C.byref(fmt) if fmt is not None else None,) if tensor else ()
        return _name(fn(None if ctx_null else gpu.ctx, None if jobs_null else t, count, *extra, None, s))

    def table(bad=None):
        t = (J * 4)()
        for i in range(4):  # level 1: the reduced image is (W / 2) x (H / 2)
            t[i] = J(dstream.data_ptr(), nbytes, W, H, Wn(8 * i, 0, 8, 8, outs[i].data_ptr(), 12, 96, 1) if tensor else Wn(8 * i, 0, 8, 8, outs[i].data_ptr(), 12, 1))
        if bad:
            bad(t[2])
        return t

    def setw(**kw):
        def f(j):
            for k, v in kw.items():
                setattr(j.window, k, v)
        return f

    def tiny(level):
        def f(j):
            j.pStream, j.streamBytes, j.sizeX, j.sizeY = dtiny.data_ptr(), tiny_bytes, 5, 3
            j.window.x0, j.window.y0, j.window.width, j.window.height, j.window.log2Scale = 0, 0, 1, 1, level
        return f

    assert call(table(), 0) == "InvalidParameter"
    assert call(table(), 4, jobs_null=True) == "ArgumentNull"
    assert call(table(), 4, ctx_null=True) == "ArgumentNull"
    if tensor:
        assert call(table(), 4, fmt=None) == "ArgumentNull" and call(table(), 0, fmt=None) == "ArgumentNull"  # (NULL before count == 0)
    stride = dict(rowStride=7) if tensor else dict(outStridePixels=7)
    cases = [
        ("log2Scale 4", setw(log2Scale=4), "InvalidParameter"),
        ("log2Scale 4 and out of bounds: the level is checked with the size", setw(log2Scale=4, x0=W), "InvalidParameter"),
        ("log2Scale 2^32 - 1", setw(log2Scale=0xFFFFFFFF), "InvalidParameter"),
        ("zero width", setw(width=0), "InvalidParameter"),
        ("zero height", setw(height=0), "InvalidParameter"),
        ("stride < width", setw(**stride), "InvalidParameter"),
        ("one pixel beyond RX", setw(x0=W // 2 - 8 + 1), "OutOfBounds"),
        ("one pixel beyond RY", setw(y0=H // 2 - 8 + 1), "OutOfBounds"),
        ("inside the image, outside the level's", setw(x0=W // 2), "OutOfBounds"),
        ("overflow", setw(x0=1 << 63, width=1 << 63, height=1, **{k: 1 << 63 for k in (("rowStride", "planeStride") if tensor else ("outStridePixels",))}), "OutOfBounds"),
        ("image smaller than k: RY == 0 at level 2", tiny(2), "OutOfBounds"),
        ("image smaller than k: RX == RY == 0 at level 3", tiny(3), "OutOfBounds"),
        ("pOut misaligned by 2", setw(pOut=outs[2].data_ptr() + 2), "InvalidParameter"),
        ("NULL pOut", setw(pOut=None), "ArgumentNull"),
        ("NULL pStream", lambda j: setattr(j, "pStream", None), "ArgumentNull"),
    ]
    if tensor:
        cases.append(("planeStride one short", setw(planeStride=7 * 12 + 8 - 1), "InvalidParameter"))
    for what, bad, code in cases:
        assert call(table(bad), 4) == code, what
        torch.cuda.synchronize()
        assert all(bool((o == SENTINEL).all()) for o in outs), what
    gpu.check()
    ok = table(tiny(1))  # the tiny image at level 1 is 2 x 1: its pixel (0, 0) exists
    assert fn(gpu.ctx, ok, 4, *((C.byref(f32),) if tensor else ()), None, s) == 0  # the context is usable afterwards
    torch.cuda.synchronize()
    gpu.check()
    planes = 3 if tensor else 1
    assert all(bool((o[:planes, :, :8] != SENTINEL).any()) and bool((o[:planes, :, 8:] == SENTINEL).all()) and bool((o[planes:] == SENTINEL).all()) for o in outs[:2] + outs[3:])
    assert bool((outs[2][:planes, 0, 0] != SENTINEL).all()) and int((outs[2] != SENTINEL).sum()) == planes
    struct_sizes()


def host_argument_errors(gpu, name, tensor, st, W, H, tiny):
    """`name`: the C symbol of a scaled host entry; st: a good stream of a W x H image; tiny: one of a 5 x 3 image"""
    fn = getattr(gpu.lib, name)
    f32 = T.fmt_of("float32", 3, "A")
    ok = np.full((3, 8, 9), SENTINEL, dtype=np.uint32)
    Wn = limg_amd.ScaledTensorWindow if tensor else limg_amd.ScaledWindow

    def win(x0=0, y0=0, width=8, height=8, out=ok.ctypes.data, stride=9, plane=72, level=1):
        return Wn(x0, y0, width, height, out, stride, plane, level) if tensor else Wn(x0, y0, width, height, out, stride, level)

    def call(stream, wins, count=None, fmt=f32):
        t = (Wn * max(1, len(wins)))(*wins) if wins is not None else None
        extra = (C.byref(fmt) if fmt is not None else None,) if tensor else ()
        return _name(fn(gpu.ctx, stream.ctypes.data if stream is not None else None, stream.size if stream is not None else 64, t, len(wins) if count is None else count, *extra))

    good = [win(), win(x0=8, y0=8)]
    assert call(st, None, count=2) == "ArgumentNull" and call(None, good) == "ArgumentNull"
    assert call(st, good, count=0) == "InvalidParameter"
    if tensor:
        assert call(st, good, fmt=None) == "ArgumentNull"
    for what, bad, code in (("log2Scale 4", win(level=4), "InvalidParameter"), ("log2Scale 4, beyond the image", win(level=4, x0=W), "InvalidParameter"),
                            ("zero width", win(width=0), "InvalidParameter"), ("stride < width", win(stride=7), "InvalidParameter"),
                            ("one pixel beyond RX", win(x0=W // 2 - 8 + 1), "OutOfBounds"), ("one pixel beyond RY at level 3", win(level=3, y0=H // 8 - 8 + 1), "OutOfBounds"),
                            ("NULL pOut", win(out=None), "ArgumentNull")):
        assert call(st, good + [bad]) == code, what
        assert (ok == SENTINEL).all(), what
    for level in (2, 3):  # 5 x 3: RY == 0 at level 2, RX == RY == 0 at level 3
        assert call(tiny, [win(width=1, height=1, level=level)]) == "OutOfBounds", level
    assert (ok == SENTINEL).all()
    gpu.check()
    assert call(tiny, [win(width=2, height=1, level=1)]) == 0  # the context is usable afterwards
    planes = 3 if tensor else 1
    assert int((ok != SENTINEL).sum()) == 2 * planes and (ok[:planes, 0, :2] != SENTINEL).all()
    gpu.check()
