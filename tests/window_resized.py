"""What the resized window decode tests of both stream versions share (limg_hip_*decode_stream_windows_resized*): the numpy statement of the contract's formula --
bilinear, align_corners = false, in integers on the level-L image of tests/window_scaled.py, clamped to the level pixels the source rectangle touches --, the job
layouts of tests/window_batch.py and tests/window_tensor.py for jobs with a source rectangle, an output size, a level and a flip, and the test bodies that do not
depend on the stream version.  A stream is (device stream, nbytes, W, H, pyramid) as in window_scaled; expected pixels never come from the library's own decode.
Everything is compared on bit patterns, in sentinel-filled outputs."""
import ctypes as C

import numpy as np

import limg_amd
import window_scaled as WS
import window_tensor as T
from window_batch import Batch
from window_cases import ERRORS, SENTINEL, windows

AUTO = None  # the level argument that lets the entry choose
OUT_SIZES = ((1, 1), (7, 5), (20, 12), (33, 9), None)  # None: 1.7 times the source, rounded up


def axis(s0, length, out, L, R, flip=False):
    """one axis of the contract: (a, b, f) for every output index; R: the level image's size along it"""
    X = np.arange(out, dtype=np.int64)
    if flip:
        X = out - 1 - X
    c16 = (np.int64(s0) << 16) + (((2 * X + 1) * length) << 15) // out
    u16 = (c16 >> L) - 32768
    i0 = u16 >> 16
    f = ((u16 & 0xFFFF) + 128) >> 8
    lo, hi = s0 >> L, min((s0 + length - 1) >> L, R - 1)
    return np.clip(i0, lo, hi), np.clip(i0 + 1, lo, hi), f


def auto_level(sw, sh, ow, oh):
    """the largest L <= 3 with (sw >> L) >= ow and (sh >> L) >= oh, 0 if none"""
    L = 0
    while L < 3 and (sw >> (L + 1)) >= ow and (sh >> (L + 1)) >= oh:
        L += 1
    return L


def level_ok(W, H, rect, L):
    """whether an explicit level accepts the rectangle: its first column and row are among those the level keeps"""
    RX, RY = W >> L, H >> L
    return RX > 0 and RY > 0 and (rect[0] >> L) <= RX - 1 and (rect[1] >> L) <= RY - 1


def resize(pyr, rect, ow, oh, level=AUTO, flip=False):
    """pyr: the pyramid of the full decode (pyr[L]: (H >> L, W >> L) uint32) -> ((oh, ow) uint32, the level used)"""
    x0, y0, sw, sh = rect
    L = auto_level(sw, sh, ow, oh) if level is None else level
    q = pyr[L]
    b = np.ascontiguousarray(q).view(np.uint8).reshape(q.shape[0], q.shape[1], 4).astype(np.int64)
    xa, xb, f = axis(x0, sw, ow, L, q.shape[1], flip)
    ya, yb, g = axis(y0, sh, oh, L, q.shape[0])
    f, g = f[None, :, None], g[:, None, None]
    top = b[ya][:, xa] * (256 - f) + b[ya][:, xb] * f
    bot = b[yb][:, xa] * (256 - f) + b[yb][:, xb] * f
    v = (top * (256 - g) + bot * g + 32768) >> 16
    assert v.min() >= 0 and v.max() <= 255
    return np.ascontiguousarray(v.astype(np.uint8)).view(np.uint32).reshape(oh, ow), L


def entry(gpu, blocked, tensor, host=False):
    return getattr(gpu, ("blocked_" if blocked else "") + "decode_stream_windows_resized" + ("_tensor" if tensor else "") + ("" if host else "_device"))


class ResizedBatch(Batch):
    """window_batch.Batch for resized jobs: a job's slice holds its oh x ow output, its expectation is resize() of the stream's pyramid"""

    def add(self, stream, rect, ow, oh, level, flip, unaligned):
        d, nbytes, W, H, pyr = stream
        k = super().add(d, nbytes, W, H, resize(pyr, rect, ow, oh, level, flip)[0], (0, 0, ow, oh), unaligned)
        self.jobs[k].update(rect=rect, level=level, flags=limg_amd.RESIZE_FLIP_X if flip else 0)
        return k

    def args(self, flat, which=None):
        return [(j["stream"], j["nbytes"], j["W"], j["H"], j["level"], j["flags"], *j["rect"], *j["win"][2:], flat[j["start"]:], j["stride"])
                for j in (self.jobs if which is None else [self.jobs[i] for i in which])]


class ResizedTensorBatch(T.TensorBatch):
    def add(self, stream, rect, ow, oh, level, flip, unaligned):
        d, nbytes, W, H, pyr = stream
        k = super().add(d, nbytes, W, H, resize(pyr, rect, ow, oh, level, flip)[0], (0, 0, ow, oh), unaligned)
        self.jobs[k].update(rect=rect, level=level, flags=limg_amd.RESIZE_FLIP_X if flip else 0)
        return k

    def args(self, flat, which=None):
        return [(j["stream"], j["nbytes"], j["W"], j["H"], j["level"], j["flags"], *j["rect"], *j["win"][2:], flat[j["start"]:], j["row"], j["plane"])
                for j in (self.jobs if which is None else [self.jobs[i] for i in which])]


def new_batch(mode):
    return ResizedBatch() if mode == "rgba" else ResizedTensorBatch(*mode)


def run(gpu, blocked, batch, mode, one_by_one=True):
    """one call over the whole layout = the expectation, sentinels included, every status word 0; the same jobs one per call give the identical buffer"""
    if mode == "rgba":
        return WS.run_rgba(gpu, entry(gpu, blocked, False), batch, one_by_one)
    return T.run_and_compare(gpu, entry(gpu, blocked, True), batch, one_by_one)


def mixed_jobs(streams):
    """(stream, rect, ow, oh, level, flip, unaligned): the rectangles of window_cases.windows as sources, the output sizes of OUT_SIZES in turn (down- and up-scaling,
    aspect changes), levels 0 .. 3 and AUTO in turn (AUTO where the explicit level would refuse the rectangle), a flip on every second job, the two placements
    alternating in pairs"""
    jobs = []
    for st in streams:
        W, H = st[2], st[3]
        for rect in windows(W, H):
            n = len(jobs)
            size = OUT_SIZES[n % len(OUT_SIZES)] or (-(-rect[2] * 17 // 10), -(-rect[3] * 17 // 10))
            level = (0, 1, 2, 3, AUTO)[(n // 2) % 5]
            if level is not None and not level_ok(W, H, rect, level):
                level = AUTO
            jobs.append((st, rect, size[0], size[1], level, bool(n & 1), bool((n >> 1) & 1)))
    return jobs


def mixed_batch(gpu, blocked, streams, mode):
    batch = new_batch(mode)
    for j in mixed_jobs(streams):
        batch.add(*j)
    assert {j["level"] for j in batch.jobs} == {0, 1, 2, 3, AUTO} and {j["flags"] for j in batch.jobs} == {0, 1}
    assert any(j["win"][2] > j["rect"][2] for j in batch.jobs) and any(j["win"][2] < j["rect"][2] for j in batch.jobs)
    run(gpu, blocked, batch, mode)


TILE_JOBS = ((0, (0, 0, None, None), 100, 60, AUTO, False), (0, (3, 1, 60, 37), 100, 60, 0, True), (1, (0, 0, None, None), 200, 8, AUTO, False),
             (1, (0, 0, None, None), 200, 8, 0, True), (1, (17, 2, 500, 16), 200, 8, 2, False))


def tiles(gpu, blocked, streams, has_hooks):
    """streams: a 72 x 40 and a 531 x 19 image.  Default capacity: the buffer equals the expectation.  Test build: with resize_tile_pixels = 64 every job splits into
    several tiles on both axes (a tile's footprint of 64 level pixels is at most 8 x 8 or a strip) and the buffer is the same"""
    import torch
    for mode in ("rgba", ("float16", 3, "A")):
        batch = new_batch(mode)
        for n, (s, (x, y, w, h), ow, oh, level, flip) in enumerate(TILE_JOBS):
            st = streams[s]
            batch.add(st, (x, y, w or st[2], h or st[3]), ow, oh, level, flip, bool(n & 1))
        a = run(gpu, blocked, batch, mode, one_by_one=False)
        if has_hooks:
            gpu.set_options(test_resize_tile_pixels=64)
            try:
                b = run(gpu, blocked, batch, mode, one_by_one=False)
            finally:
                gpu.set_options()
            assert torch.equal(a, b)


def identity_level_flip(gpu, blocked, streams):
    """identity (out == source size, level 0, no flip) = the batched window entry; rectangles and sizes in multiples of k at 1 / k = the scaled entry, explicitly and by
    AUTO; the flip = the column reversal of the unflipped job: all bit for bit, against what those entries WRITE (and, through the batch, against the oracle)"""
    import torch
    plain = getattr(gpu, ("blocked_" if blocked else "") + "decode_stream_windows_device")
    scaled = WS.entry(gpu, blocked, False)
    resized = entry(gpu, blocked, False)
    for st in streams:
        d, nbytes, W, H, pyr = st
        batch = ResizedBatch()
        for i, rect in enumerate(windows(W, H)):
            batch.add(st, rect, rect[2], rect[3], 0, False, bool(i & 1))
        a = run(gpu, blocked, batch, "rgba", one_by_one=False)
        b = torch.full_like(a, SENTINEL)
        plain([(d, nbytes, W, H, *j["rect"], b[j["start"]:], j["stride"]) for j in batch.jobs])
        torch.cuda.synchronize()
        assert torch.equal(a, b), "identity"
        for L in (1, 2, 3):
            k = 1 << L
            RX, RY = W >> L, H >> L
            if RX < 2 or RY < 2:
                continue
            for level in (L, AUTO):
                batch = ResizedBatch()
                for i, (x, y, w, h) in enumerate(windows(RX, RY)):
                    batch.add(st, (x * k, y * k, w * k, h * k), w, h, level, False, bool(i & 1))
                a = run(gpu, blocked, batch, "rgba", one_by_one=False)
                b = torch.full_like(a, SENTINEL)
                scaled([(d, nbytes, W, H, L, j["rect"][0] // k, j["rect"][1] // k, *j["win"][2:], b[j["start"]:], j["stride"]) for j in batch.jobs])
                torch.cuda.synchronize()
                assert torch.equal(a, b), ("pure level", L, level)
        jobs = [(rect, ow, oh, level) for rect, (ow, oh), level in zip(windows(W, H)[5:], ((20, 12), (33, 9), (7, 5), (50, 31), (9, 40), (64, 3), (65, 2)), (AUTO, 0, AUTO, 1, 0, AUTO, 0))
                if level is None or level_ok(W, H, rect, level)]
        straight = resized([(d, nbytes, W, H, level, 0, *rect, ow, oh, None, None) for rect, ow, oh, level in jobs])
        mirrored = resized([(d, nbytes, W, H, level, limg_amd.RESIZE_FLIP_X, *rect, ow, oh, None, None) for rect, ow, oh, level in jobs])
        torch.cuda.synchronize()
        for job, s, m in zip(jobs, straight, mirrored):
            assert torch.equal(m, torch.flip(s, dims=(1,))), ("flip", job)
            assert np.array_equal(s.cpu().numpy().view(np.uint32), resize(pyr, *job)[0]), job
    gpu.check()


def ragged_edges(gpu, blocked, big, tiny):
    """rectangles that touch the right and the bottom edge at levels 1 .. 3, where the level drops trailing columns and rows: the taps clamp to the last level pixel"""
    batch = ResizedBatch()
    for st in (big, tiny):
        W, H = st[2], st[3]
        rects = [(W - w, H - h, w, h) for w, h in ((W, H), (min(W, 37), min(H, 16)), (min(W, 11), min(H, 3)), (1, 1), (W, 1), (1, H))]
        for L in (1, 2, 3):
            for i, rect in enumerate(rects):
                if level_ok(W, H, rect, L):
                    for ow, oh in ((rect[2], rect[3]), (13, 7), (max(1, rect[2] >> L), max(1, rect[3] >> L))):
                        batch.add(st, rect, ow, oh, L, bool(i & 1), bool(len(batch.jobs) & 1))
    assert {j["level"] for j in batch.jobs} == {1, 2, 3} and any(j["W"] == tiny[2] for j in batch.jobs)
    run(gpu, blocked, batch, "rgba", one_by_one=False)


def tensor_equals_conversion_of_rgba(gpu, blocked, stream):
    import torch
    d, nbytes, W, H, pyr = stream
    jobs = [(AUTO, 0, 0, 0, W, H, 20, 12), (0, 1, 3, 2, W - 5, H - 4, 33, 9), (1, 0, 2, 2, W - 2, H - 2, 31, 17), (AUTO, 1, 1, 1, 40, 30, 68, 51), (2, 1, 0, 0, W, H, 9, 9)]
    rgba = entry(gpu, blocked, False)([(d, nbytes, W, H, *j, None, None) for j in jobs])
    torch.cuda.synchronize()
    rgba = [r.cpu().numpy().view(np.uint32) for r in rgba]
    for (level, flags, x, y, sw, sh, ow, oh), r in zip(jobs, rgba):
        assert np.array_equal(r, resize(pyr, (x, y, sw, sh), ow, oh, level, bool(flags))[0]), (level, flags, x, y, sw, sh, ow, oh)
    for dtype, planes, consts in T.FORMATS:
        got = entry(gpu, blocked, True)([(d, nbytes, W, H, *j, None, None, None) for j in jobs], T.fmt_of(dtype, planes, consts))
        torch.cuda.synchronize()
        for job, r, g in zip(jobs, rgba, got):
            assert np.array_equal(g.cpu().numpy().view(T.BITS[dtype]), T.convert(r, dtype, planes, consts).view(T.BITS[dtype])), (job, dtype, planes, consts)
    gpu.check()


def crops(gpu, blocked, streams, dtype, planes):
    """decode_crops_resized_device: 18 random rectangles of three streams to 20 x 12, every second one mirrored, AUTO and explicit levels, into its own tensor and into a
    caller's tensor with a sentinel slice behind it = the stacked numpy expectation"""
    import torch
    tb, tf = T._torch_bits(dtype)
    rng = np.random.RandomState(13)
    scale, bias = T.CONSTANTS["A"]
    for level in (AUTO, 0):
        jobs, want = [], []
        for i in range(18):
            st = streams[i % 3]
            d, nbytes, W, H, pyr = st
            sw, sh = int(rng.randint(8, W + 1)), int(rng.randint(6, H + 1))
            x, y = int(rng.randint(0, W - sw + 1)), int(rng.randint(0, H - sh + 1))
            jobs.append((d, nbytes, W, H, x, y, sw, sh) + ((True,) if i & 1 else (False,) if i & 2 else ()))
            want.append(torch.from_numpy(T.convert(resize(pyr, (x, y, sw, sh), 20, 12, level, bool(i & 1))[0], dtype, planes, "A")))
        out = gpu.decode_crops_resized_device(jobs, 12, 20, tf, scale[:planes], bias[:planes], planes=planes, blocked=blocked, level=level)
        torch.cuda.synchronize()
        assert tuple(out.shape) == (18, planes, 12, 20) and out.is_contiguous() and out.dtype == tf
        assert torch.equal(out.cpu().view(tb), torch.stack(want).view(tb)), level
        bits, flat = T.sentinel_tensor((19, planes, 12, 20), dtype)
        assert gpu.decode_crops_resized_device(jobs, 12, 20, tf, scale[:planes], bias[:planes], planes=planes, blocked=blocked, out=flat[:18], level=level).data_ptr() == flat.data_ptr()
        torch.cuda.synchronize()
        assert torch.equal(bits[:18].cpu(), torch.stack(want).view(tb)) and bool((bits[18] == T.SENT[dtype]).all())
    gpu.check()


def back_to_back(gpu, blocked, stream):
    """six calls issued without synchronising, RGBA and tensor alternating -- more than the ring's four slots"""
    import torch
    first, second = ResizedBatch(), ResizedTensorBatch("float16", 4, "B")
    for j in mixed_jobs([stream]):
        first.add(*j)
        second.add(*j[:5], not j[5], not j[6])
    (f1, e1), (b2, f2, e2) = first.tensors(), second.tensors()
    a1, a2, m2 = first.args(f1), second.args(f2), T.fmt_of("float16", 4, "B")
    torch.cuda.synchronize()
    for _ in range(3):
        entry(gpu, blocked, False)(a1)
        entry(gpu, blocked, True)(a2, m2)
    torch.cuda.synchronize()
    assert torch.equal(f1, e1) and torch.equal(b2, e2)
    gpu.check()


def _host_wins(W, H):
    """(level, flags, x, y, sw, sh, ow, oh)"""
    return [(AUTO, 0, 0, 0, W, H, 20, 12), (0, 1, 1, 1, W - 3, H - 2, 31, 7), (1, 0, 0, 0, W, H, W // 3, max(1, H // 3)), (AUTO, 1, W // 4, 0, W // 2, H, 9, 5),
            (0, 0, 2, 1, min(W - 2, 20), min(H - 1, 9), 34, 15)]


def host_forms(gpu, blocked, st, W, H, pyr):
    """one call for all windows of a stream, each into the middle of a sentinel array with slack: RGBA, then two tensor formats; outs=None allocates"""
    wins = _host_wins(W, H)
    want = [resize(pyr, (x, y, sw, sh), ow, oh, level, bool(flags))[0] for level, flags, x, y, sw, sh, ow, oh in wins]
    bufs = [np.full((w[7] + 3, w[6] + 7), SENTINEL, dtype=np.uint32) for w in wins]
    got = entry(gpu, blocked, False, host=True)(st, wins, outs=[b[1:1 + w[7], 2:2 + w[6]] for b, w in zip(bufs, wins)])
    assert len(got) == len(wins)
    for b, w, e in zip(bufs, wins, want):
        exp = np.full_like(b, SENTINEL)
        exp[1:1 + w[7], 2:2 + w[6]] = e
        assert np.array_equal(b, exp), (w, np.argwhere(b != exp)[:6].tolist())
    for dtype, planes, consts in (("float32", 3, "A"), ("float16", 4, "B")):
        bufs = [np.full((planes + 1, w[7] + 3, w[6] + 7), T.SENT[dtype], dtype=T.BITS[dtype]) for w in wins]
        entry(gpu, blocked, True, host=True)(st, wins, T.fmt_of(dtype, planes, consts), outs=[b.view(T.NP[dtype])[:planes, 1:1 + w[7], 2:2 + w[6]] for b, w in zip(bufs, wins)])
        for b, w, e in zip(bufs, wins, want):
            exp = np.full_like(b, T.SENT[dtype])
            exp[:planes, 1:1 + w[7], 2:2 + w[6]] = T.convert(e, dtype, planes, consts).view(T.BITS[dtype])
            assert np.array_equal(b, exp), (w, dtype, np.argwhere(b != exp)[:6].tolist())
    got = entry(gpu, blocked, False, host=True)(st, wins[:1])
    assert np.array_equal(got[0], want[0])
    gpu.check()


def host_forms_refused(gpu, blocked, evil, wins):
    """a stream that is refused for one window: the call raises and EVERY output is untouched, RGBA and tensor"""
    import pytest
    bufs = [np.full((w[7], w[6] + 3), SENTINEL, dtype=np.uint32) for w in wins]
    with pytest.raises(limg_amd.LimgHipError):
        entry(gpu, blocked, False, host=True)(evil, wins, outs=[b[:, :w[6]] for b, w in zip(bufs, wins)])
        pytest.fail("accepted")
    assert all((b == SENTINEL).all() for b in bufs)
    gpu.check()
    bufs = [np.full((3, w[7], w[6] + 3), T.SENT["float32"], dtype=np.int32) for w in wins]
    with pytest.raises(limg_amd.LimgHipError):
        entry(gpu, blocked, True, host=True)(evil, wins, T.fmt_of("float32", 3, "A"), outs=[b.view(np.float32)[:, :, :w[6]] for b, w in zip(bufs, wins)])
        pytest.fail("accepted")
    assert all((b == T.SENT["float32"]).all() for b in bufs)
    gpu.check()


def _name(r):
    return {v: k for k, v in ERRORS.items()}.get(r, r)


def struct_sizes():
    z = C.sizeof(C.c_size_t)
    assert C.sizeof(limg_amd.ResizedWindow) == 9 * z and C.sizeof(limg_amd.ResizedWindowJob) == 13 * z
    assert C.sizeof(limg_amd.ResizedTensorWindow) == 10 * z and C.sizeof(limg_amd.ResizedTensorWindowJob) == 14 * z
    assert limg_amd.ResizedWindow.outWidth.offset == 6 * z and limg_amd.ResizedWindow.log2Scale.offset == 8 * z and limg_amd.ResizedWindow.flags.offset == 8 * z + 4
    assert limg_amd.ResizedTensorWindow.outWidth.offset == 7 * z and limg_amd.ResizedTensorWindow.flags.offset == 9 * z + 4


# the contract's error list as (what, window members to set, code); W, H: the good stream's image (at least 64 x 64)
def _error_cases(W, H, tensor, misaligned):
    stride = dict(rowStride=7) if tensor else dict(outStridePixels=7)
    cases = [
        ("log2Scale 4", dict(log2Scale=4), "InvalidParameter"),
        ("log2Scale 4 and out of bounds: the level is checked with the size", dict(log2Scale=4, x0=W), "InvalidParameter"),
        ("log2Scale 2^32 - 2", dict(log2Scale=0xFFFFFFFE), "InvalidParameter"),
        ("flag bit 1", dict(flags=2), "InvalidParameter"),
        ("flag bit 31 with bit 0", dict(flags=0x80000001), "InvalidParameter"),
        ("zero width", dict(width=0), "InvalidParameter"),
        ("zero height", dict(height=0), "InvalidParameter"),
        ("zero outWidth", dict(outWidth=0), "InvalidParameter"),
        ("zero outHeight", dict(outHeight=0), "InvalidParameter"),
        ("outWidth 32769", dict(outWidth=32769, **{k: 40000 for k in stride}), "InvalidParameter"),
        ("outHeight 32769", dict(outHeight=32769, **({"planeStride": 1 << 40} if tensor else {})), "InvalidParameter"),
        ("stride < outWidth", dict(**stride), "InvalidParameter"),
        ("source one pixel beyond the image", dict(x0=W - 16 + 1), "OutOfBounds"),
        ("source below the image", dict(y0=H), "OutOfBounds"),
        ("overflow", dict(x0=1 << 63, width=1 << 63), "OutOfBounds"),
        ("explicit level, rectangle starts in the dropped columns", None, "OutOfBounds"),  # (the tiny image: see the callers)
        ("explicit level, RY == 0", None, "OutOfBounds"),
        ("NULL pOut", dict(pOut=None), "ArgumentNull"),
    ]
    if misaligned is not None:
        cases.append(("pOut misaligned by 2", dict(pOut=misaligned), "InvalidParameter"))
    if tensor:
        cases.append(("planeStride one short", dict(planeStride=7 * 12 + 8 - 1), "InvalidParameter"))
    return cases


def device_argument_errors(gpu, name, tensor, dstream, nbytes, W, H, dtiny, tiny_bytes):
    """`name`: the C symbol of a resized device entry; dstream: a good stream of a W x H image (W, H >= 64); dtiny: a good stream of a 5 x 3 image.  NULL and count 0 in
    the documented order; each case of the contract's list as job 2 of 4: the right code comes back and nothing was enqueued -- all four outputs still hold the
    sentinel; then a good list decodes"""
    import torch
    fn = getattr(gpu.lib, name)
    s = gpu._stream()
    f32 = T.fmt_of("float32", 3, "A")
    outs = [torch.full((3, 8, 12), SENTINEL, dtype=torch.int32, device="cuda") for _ in range(4)]
    J, Wn = (limg_amd.ResizedTensorWindowJob, limg_amd.ResizedTensorWindow) if tensor else (limg_amd.ResizedWindowJob, limg_amd.ResizedWindow)

    def call(t, count, jobs_null=False, ctx_null=False, fmt=f32):
        extra = (C.byref(fmt) if fmt is not None else None,) if tensor else ()
        return _name(fn(None if ctx_null else gpu.ctx, None if jobs_null else t, count, *extra, None, s))

    def table(bad=None):
        t = (J * 4)()
        for i in range(4):  # a 16 x 16 source at level 1 to 8 x 8
            t[i] = J(dstream.data_ptr(), nbytes, W, H, Wn(16 * i, 0, 16, 16, outs[i].data_ptr(), 12, 96, 8, 8, 1, i & 1) if tensor else Wn(16 * i, 0, 16, 16, outs[i].data_ptr(), 12, 8, 8, 1, i & 1))
        if bad:
            bad(t[2])
        return t

    def setw(**kw):
        def f(j):
            for k, v in kw.items():
                setattr(j.window, k, v)
        return f

    def tiny(level, x0=0, width=1):
        def f(j):
            j.pStream, j.streamBytes, j.sizeX, j.sizeY = dtiny.data_ptr(), tiny_bytes, 5, 3
            j.window.x0, j.window.y0, j.window.width, j.window.height, j.window.log2Scale, j.window.outWidth, j.window.outHeight = x0, 0, width, 1, level, 1, 1
        return f

    assert call(table(), 0) == "InvalidParameter"
    assert call(table(), 4, jobs_null=True) == "ArgumentNull"
    assert call(table(), 4, ctx_null=True) == "ArgumentNull"
    if tensor:
        assert call(table(), 4, fmt=None) == "ArgumentNull" and call(table(), 0, fmt=None) == "ArgumentNull"
    for what, members, code in _error_cases(W, H, tensor, outs[2].data_ptr() + 2) + [("NULL pStream", "pStream", "ArgumentNull")]:
        if members == "pStream":
            bad = lambda j: setattr(j, "pStream", None)
        elif members is None:
            bad = tiny(1, x0=4) if "columns" in what else tiny(2)  # 5 x 3: level 1 is 2 x 1, so column 4 is dropped; at level 2 RY == 0
        else:
            bad = setw(**members)
        assert call(table(bad), 4) == code, what
        torch.cuda.synchronize()
        assert all(bool((o == SENTINEL).all()) for o in outs), what
    gpu.check()
    ok = table(tiny(1, width=5))  # the tiny image's whole first row at level 1: one output pixel
    assert fn(gpu.ctx, ok, 4, *((C.byref(f32),) if tensor else ()), None, s) == 0  # the context is usable afterwards
    torch.cuda.synchronize()
    gpu.check()
    planes = 3 if tensor else 1
    assert all(bool((o[:planes, :, :8] != SENTINEL).any()) and bool((o[:planes, :, 8:] == SENTINEL).all()) and bool((o[planes:] == SENTINEL).all()) for o in outs[:2] + outs[3:])
    assert bool((outs[2][:planes, 0, 0] != SENTINEL).all()) and int((outs[2] != SENTINEL).sum()) == planes
    struct_sizes()


def host_argument_errors(gpu, name, tensor, st, W, H, tiny):
    """`name`: the C symbol of a resized host entry; st: a good stream of a W x H image; tiny: one of a 5 x 3 image"""
    fn = getattr(gpu.lib, name)
    f32 = T.fmt_of("float32", 3, "A")
    ok = np.full((3, 8, 9), SENTINEL, dtype=np.uint32)
    Wn = limg_amd.ResizedTensorWindow if tensor else limg_amd.ResizedWindow
    names = [k for k, _ in Wn._fields_]

    def win(**kw):
        v = dict(x0=0, y0=0, width=16, height=16, pOut=ok.ctypes.data, outWidth=8, outHeight=8, log2Scale=1, flags=0)
        v.update(dict(rowStride=9, planeStride=72) if tensor else dict(outStridePixels=9))
        v.update(kw)
        return Wn(*[v[k] for k in names])

    def call(stream, wins, count=None, fmt=f32):
        t = (Wn * max(1, len(wins)))(*wins) if wins is not None else None
        extra = (C.byref(fmt) if fmt is not None else None,) if tensor else ()
        return _name(fn(gpu.ctx, stream.ctypes.data if stream is not None else None, stream.size if stream is not None else 64, t, len(wins) if count is None else count, *extra))

    good = [win(), win(x0=16, y0=16, flags=1)]
    assert call(st, None, count=2) == "ArgumentNull" and call(None, good) == "ArgumentNull"
    assert call(st, good, count=0) == "InvalidParameter"
    if tensor:
        assert call(st, good, fmt=None) == "ArgumentNull"
    for what, members, code in _error_cases(W, H, tensor, None):
        if members is None:
            continue
        if "planeStride" in members and members.get("planeStride") == 7 * 12 + 8 - 1:
            members = dict(planeStride=7 * 9 + 8 - 1)
        assert call(st, good + [win(**members)]) == code, what
        assert (ok == SENTINEL).all(), what
    assert call(tiny, [win(x0=4, width=1, height=1, outWidth=1, outHeight=1)]) == "OutOfBounds"  # level 1 of 5 x 3 is 2 x 1: column 4 is dropped
    assert call(tiny, [win(width=1, height=1, outWidth=1, outHeight=1, log2Scale=2)]) == "OutOfBounds"  # RY == 0
    assert (ok == SENTINEL).all()
    gpu.check()
    assert call(tiny, [win(width=5, height=3, outWidth=2, outHeight=1, log2Scale=limg_amd.RESIZE_AUTO)]) == 0  # the context is usable afterwards
    planes = 3 if tensor else 1
    assert int((ok != SENTINEL).sum()) == 2 * planes and (ok[:planes, 0, :2] != SENTINEL).all()
    gpu.check()
