"""What the tensor window decode tests of both stream versions share (limg_hip_*decode_stream_windows_tensor*): the Batch of tests/window_batch.py for planar float
output -- many jobs laid out as disjoint slices of ONE sentinel-filled flat device tensor, aligned and misaligned placements for both element types, a plane stride
larger than height * rowStride in half the jobs -- the numpy statement of the contract's conversion, and the test bodies that do not depend on the stream version.
Everything is compared on BIT PATTERNS (int32 / int16 views): -0.0 and NaN payloads cannot hide anything, and the sentinel is a bit pattern too."""
import ctypes as C

import numpy as np

import limg_amd
from window_cases import ERRORS, windows

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
# (A) the usual normalisation, channel 3 as 1/255: every result is 0 or of magnitude 0.0039 .. 2.64, so nothing is subnormal and nothing overflows in float16;
# (B) exact in both types
CONSTANTS = {"A": ([1 / (255 * s) for s in STD] + [1 / 255], [-m / s for m, s in zip(MEAN, STD)] + [0.0]), "B": ([1.0] * 4, [-128.0] * 4)}
NP = {"float32": np.float32, "float16": np.float16}
BITS = {"float32": np.int32, "float16": np.int16}
SENT = {"float32": 0x5A5A5A5A, "float16": 0x5A5A}
FORMATS = [(d, p, k) for d in ("float32", "float16") for p in (3, 4) for k in ("A", "B")]


def fmt_of(dtype, planes, consts):
    scale, bias = CONSTANTS[consts]
    return limg_amd.tensor_format(dtype, planes, scale, bias)


def convert(pixels, dtype, planes, consts):
    """(h, w) uint32 pixels -> (planes, h, w) of dtype, as the contract states it: float32 multiply, then float32 add, then (float16) round to nearest even"""
    scale, bias = CONSTANTS[consts]
    out = np.empty((planes,) + pixels.shape, NP[dtype])
    for c in range(planes):
        b = ((pixels >> np.uint32(8 * c)) & np.uint32(0xFF)).astype(np.float32)
        out[c] = ((b * np.float32(scale[c])) + np.float32(bias[c])).astype(NP[dtype])
    return out


def _torch_bits(dtype):
    import torch
    return {"float32": (torch.int32, torch.float32), "float16": (torch.int16, torch.float16)}[dtype]


def sentinel_tensor(shape, dtype):
    """(bits view, float view) of one sentinel-filled device tensor"""
    import torch
    tb, tf = _torch_bits(dtype)
    bits = torch.full(shape, SENT[dtype], dtype=tb, device="cuda")
    return bits, bits.view(tf)


class TensorBatch:
    """add() jobs, then tensors(): (bits, flat, expected bits).  A job's slice starts 16-byte aligned with row and plane strides that are multiples of 16 bytes (so
    pieces at x0 % (16 / element size) == 0 take the 16-byte stores) or, unaligned, one element off a 16-byte boundary with an odd row stride (every piece leaves
    element by element).  Jobs 2, 3, 6, 7, ... have a plane stride larger than height * rowStride.  Between and around the slices, in every row's slack and between the
    planes the sentinel must survive."""

    def __init__(self, dtype, planes, consts):
        self.dtype, self.planes, self.consts = dtype, planes, consts
        self.per = 16 // np.dtype(NP[dtype]).itemsize
        self.jobs, self.off = [], 2 * self.per

    def add(self, dstream, nbytes, W, H, want, win, unaligned):
        x, y, w, h = win
        per, k = self.per, len(self.jobs)
        row = (w + 5) | 1 if unaligned else (w + per) // per * per
        plane = h * row + (0 if k % 4 < 2 else (3 if unaligned else 2 * per))
        start = (self.off + per - 1) // per * per + per + (1 if unaligned else 0)
        self.off = start + (self.planes - 1) * plane + h * row + 3
        self.jobs.append(dict(stream=dstream, nbytes=nbytes, W=W, H=H, want=want, win=win, row=row, plane=plane, start=start))
        return k

    def tensors(self):
        import torch
        n = self.off + 2 * self.per
        bits, flat = sentinel_tensor((n,), self.dtype)
        assert flat.data_ptr() % 16 == 0
        exp = np.full(n, SENT[self.dtype], dtype=BITS[self.dtype])
        for j in self.jobs:
            x, y, w, h = j["win"]
            v = convert(j["want"][y:y + h, x:x + w], self.dtype, self.planes, self.consts).view(BITS[self.dtype])
            for c in range(self.planes):
                at = j["start"] + c * j["plane"]
                exp[at:at + h * j["row"]].reshape(h, j["row"])[:, :w] = v[c]
        return bits, flat, torch.from_numpy(exp).cuda()

    def args(self, flat, which=None):
        """the job tuples of LimgHip.*decode_stream_windows_tensor_device, writing into `flat`"""
        return [(j["stream"], j["nbytes"], j["W"], j["H"], *j["win"], flat[j["start"]:], j["row"], j["plane"]) for j in (self.jobs if which is None else [self.jobs[i] for i in which])]

    def slice_of(self, bits, i):
        """job i's window in `bits` as numpy (planes, h, w) bit patterns"""
        j = self.jobs[i]
        x, y, w, h = j["win"]
        t = bits.cpu().numpy()
        return np.stack([t[j["start"] + c * j["plane"]:][:h * j["row"]].reshape(h, j["row"])[:, :w] for c in range(self.planes)])


def run_and_compare(gpu, entry, batch, one_by_one=True):
    """One call over the whole layout: the tensor equals the expected one everywhere, sentinels included; pJobStatus is all 0; the same jobs issued one per call give
    the identical tensor.  entry: the LimgHip method.  Returns the bits."""
    import torch
    fmt = fmt_of(batch.dtype, batch.planes, batch.consts)
    bits, flat, exp = batch.tensors()
    status = torch.full((len(batch.jobs),), 77, dtype=torch.int32, device="cuda")
    entry(batch.args(flat), fmt, status=status)
    torch.cuda.synchronize()
    bad = torch.nonzero(bits != exp)[:6].ravel().tolist()
    assert not bad, (bad, [(i, j["win"], j["start"], j["row"], j["plane"]) for i, j in enumerate(batch.jobs)
                           if any(j["start"] - 8 <= b <= j["start"] + batch.planes * j["plane"] + 8 for b in bad)][:4])
    assert not bool(status.any()), status.cpu().tolist()
    if one_by_one:
        bits1, flat1 = sentinel_tensor(tuple(bits.shape), batch.dtype)
        for a in batch.args(flat1):
            entry([a], fmt)
        torch.cuda.synchronize()
        assert torch.equal(bits1, bits)
    gpu.check()
    return bits


def mixed_batch(gpu, entry, streams, dtype, planes, consts):
    """streams: (device stream, nbytes, W, H, pDecoded) each: every window of windows(W, H) of every image in ONE call, aligned and misaligned jobs alternating"""
    batch = TensorBatch(dtype, planes, consts)
    for d, nbytes, W, H, want in streams:
        for win in windows(W, H):
            batch.add(d, nbytes, W, H, want, win, unaligned=bool(len(batch.jobs) & 1))
    assert any(j["plane"] > j["win"][3] * j["row"] for j in batch.jobs[0::2]) and any(j["plane"] > j["win"][3] * j["row"] for j in batch.jobs[1::2])
    run_and_compare(gpu, entry, batch)


def store_paths_agree(gpu, entry, stream, dtype):
    """a window with x0 % 8 == 0 and one with x0 % 8 == 4, each into an aligned and a misaligned slice: equal values in both placements.  The aligned x0 % 8 == 4 job
    takes the 16-byte stores for float32 and the element stores for float16."""
    d, nbytes, W, H, want = stream
    for planes in (3, 4):
        batch = TensorBatch(dtype, planes, "A")
        for win in ((8, 3, 40, 12), (12, 3, 40, 12)):
            for unaligned in (False, True, False, True):  # (with and without plane slack)
                batch.add(d, nbytes, W, H, want, win, unaligned)
        bits = run_and_compare(gpu, entry, batch)
        for base in (0, 4):
            got = [batch.slice_of(bits, base + i) for i in range(4)]
            assert all(np.array_equal(got[0], g) for g in got[1:])


def many_tiny_jobs(gpu, entry, stream, dtype):
    """300 jobs of 1 x 1, single-row and small windows on one 256 x 64 stream"""
    d, nbytes, W, H, want = stream
    assert (W, H) == (256, 64)
    rng = np.random.RandomState(5)
    batch = TensorBatch(dtype, 3, "A")
    for i in range(300):
        if i % 3 == 0:
            win = (int(rng.randint(0, 256)), int(rng.randint(0, 64)), 1, 1)
        elif i % 3 == 1:
            x = int(rng.randint(0, 256))
            win = (x, int(rng.randint(0, 64)), int(rng.randint(1, 257 - x)), 1)
        else:
            x, y = int(rng.randint(0, 256)), int(rng.randint(0, 64))
            win = (x, y, int(rng.randint(1, min(40, 256 - x) + 1)), int(rng.randint(1, min(20, 64 - y) + 1)))
        batch.add(d, nbytes, W, H, want, win, unaligned=bool(i & 1))
    run_and_compare(gpu, entry, batch, one_by_one=False)


def nchw_batch(gpu, streams, blocked, dtype, planes):
    """decode_crops_device: 24 crops of 40 x 24 out of three streams into one contiguous tensor = torch.stack of the numpy conversions"""
    import torch
    assert len(streams) == 3
    tb, tf = _torch_bits(dtype)
    rng = np.random.RandomState(7)
    jobs, want = [], []
    for i in range(24):
        d, nbytes, W, H, dec = streams[i % 3]
        x, y = int(rng.randint(0, W - 40 + 1)), int(rng.randint(0, H - 24 + 1))
        if i % 4 == 0:
            x = x // 8 * 8
        jobs.append((d, nbytes, W, H, x, y))
        want.append(torch.from_numpy(convert(dec[y:y + 24, x:x + 40], dtype, planes, "A")))
    scale, bias = CONSTANTS["A"]
    out = gpu.decode_crops_device(jobs, 24, 40, tf, scale[:planes], bias[:planes], planes=planes, blocked=blocked)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (24, planes, 24, 40) and out.is_contiguous() and out.dtype == tf
    assert torch.equal(out.cpu().view(tb), torch.stack(want).view(tb))
    # into a tensor of the caller's
    bits, flat = sentinel_tensor((25, planes, 24, 40), dtype)
    assert gpu.decode_crops_device(jobs, 24, 40, tf, scale[:planes], bias[:planes], planes=planes, blocked=blocked, out=flat[:24]).data_ptr() == flat.data_ptr()
    torch.cuda.synchronize()
    assert torch.equal(bits[:24].cpu(), torch.stack(want).view(tb)) and bool((bits[24] == SENT[dtype]).all())
    gpu.check()


def back_to_back(gpu, entry, stream):
    """six calls issued without synchronising, more than the ring's four slots: both layouts come out correct"""
    import torch
    d, nbytes, W, H, want = stream
    first, second = TensorBatch("float32", 3, "A"), TensorBatch("float16", 4, "B")
    for i, win in enumerate(windows(W, H)):
        first.add(d, nbytes, W, H, want, win, unaligned=bool(i & 1))
    for i, win in enumerate(windows(W, H, seed=2)[::-1] + [(3, 3, W - 6, H - 4)]):
        second.add(d, nbytes, W, H, want, win, unaligned=not (i & 1))
    (b1, f1, e1), (b2, f2, e2) = first.tensors(), second.tensors()
    a1, a2 = first.args(f1), second.args(f2)
    m1, m2 = fmt_of("float32", 3, "A"), fmt_of("float16", 4, "B")
    torch.cuda.synchronize()
    for _ in range(3):
        entry(a1, m1)
        entry(a2, m2)
    torch.cuda.synchronize()
    assert torch.equal(b1, e1) and torch.equal(b2, e2)
    gpu.check()


def host_windows(decode, stream, want, wins, dtype, planes, consts):
    """The host form: every window into the middle of a sentinel-filled array of its own, with row slack, plane slack and one plane more than the format has"""
    fmt = fmt_of(dtype, planes, consts)
    bufs = [np.full((planes + 1, h + 3, w + 7), SENT[dtype], dtype=BITS[dtype]) for x, y, w, h in wins]
    got = decode(stream, wins, fmt, outs=[b.view(NP[dtype])[:planes, 1:1 + h, 2:2 + w] for b, (x, y, w, h) in zip(bufs, wins)])
    assert len(got) == len(wins)
    for b, (x, y, w, h) in zip(bufs, wins):
        exp = np.full_like(b, SENT[dtype])
        exp[:planes, 1:1 + h, 2:2 + w] = convert(want[y:y + h, x:x + w], dtype, planes, consts).view(BITS[dtype])
        assert np.array_equal(b, exp), ((x, y, w, h), np.argwhere(b != exp)[:6].tolist())


def host_windows_refused(decode, stream, wins, dtype="float32", planes=3):
    """a stream that is refused for one window: the call raises and EVERY output is untouched"""
    import pytest
    fmt = fmt_of(dtype, planes, "A")
    bufs = [np.full((planes, h, w + 3), SENT[dtype], dtype=BITS[dtype]) for x, y, w, h in wins]
    with pytest.raises(limg_amd.LimgHipError):
        decode(stream, wins, fmt, outs=[b.view(NP[dtype])[:, :, :w] for b, (x, y, w, h) in zip(bufs, wins)])
        pytest.fail("accepted")
    assert all((b == SENT[dtype]).all() for b in bufs)


def _name(r):
    return {v: k for k, v in ERRORS.items()}.get(r, r)


def argument_errors(gpu, entry, dstream, nbytes, W, H):
    """NULL and empty lists, a bad format; job 2 of 4 bad in each way the single-window rules and the tensor entries' own reject: the right code comes back, and nothing
    was enqueued -- all four outputs still hold the sentinel.  Then a good list decodes.  `entry`: the C symbol's name; dstream: a good stream of a W x H image."""
    import torch
    fn = getattr(gpu.lib, entry)
    s = gpu._stream()
    outs = [sentinel_tensor((3, 8, 12), "float32") for _ in range(4)]
    f32, f16 = fmt_of("float32", 3, "A"), fmt_of("float16", 3, "A")
    J, Wn = limg_amd.TensorWindowJob, limg_amd.TensorWindow

    def table(bad=None):
        t = (J * 4)()
        for i in range(4):
            t[i] = J(dstream.data_ptr(), nbytes, W, H, Wn(8 * i, 0, 8, 8, outs[i][1].data_ptr(), 12, 96))
        if bad:
            bad(t[2])
        return t

    def setw(**kw):
        def f(j):
            for k, v in kw.items():
                setattr(j.window, k, v)
        return f

    def fmt(**kw):
        f = fmt_of("float32", 3, "A")
        for k, v in kw.items():
            setattr(f, k, v)
        return f

    def untouched(what):
        torch.cuda.synchronize()
        assert all(bool((b == SENT["float32"]).all()) for b, _ in outs), what

    assert _name(fn(gpu.ctx, table(), 0, C.byref(f32), None, s)) == "InvalidParameter"
    assert _name(fn(gpu.ctx, None, 4, C.byref(f32), None, s)) == "ArgumentNull"
    assert _name(fn(None, table(), 4, C.byref(f32), None, s)) == "ArgumentNull"
    assert _name(fn(gpu.ctx, table(), 4, None, None, s)) == "ArgumentNull"
    assert _name(fn(gpu.ctx, table(), 0, None, None, s)) == "ArgumentNull"  # (NULL before count == 0)
    for what, f in (("type 2", fmt(type=2)), ("planes 2", fmt(planes=2)), ("planes 5", fmt(planes=5))):
        assert _name(fn(gpu.ctx, table(), 4, C.byref(f), None, s)) == "InvalidParameter", what
        untouched(what)
    assert _name(fn(gpu.ctx, table(setw(pOut=None)), 4, C.byref(fmt(type=2)), None, s)) == "InvalidParameter"  # (the format before the jobs)
    cases = [
        ("zero width", setw(width=0), "InvalidParameter", f32),
        ("zero height", setw(height=0), "InvalidParameter", f32),
        ("rowStride < width", setw(rowStride=7), "InvalidParameter", f32),
        ("planeStride one short", setw(planeStride=7 * 12 + 8 - 1), "InvalidParameter", f32),
        ("out of bounds", setw(x0=W - 4), "OutOfBounds", f32),
        ("below the image", setw(y0=H), "OutOfBounds", f32),
        ("overflow", setw(x0=1 << 63, width=1 << 63, height=1, rowStride=1 << 63, planeStride=1 << 63), "OutOfBounds", f32),
        ("stride product overflows", setw(rowStride=1 << 62, planeStride=8), "InvalidParameter", f32),
        ("pOut off by 2 bytes, float32", setw(pOut=outs[2][1].data_ptr() + 2), "InvalidParameter", f32),
        ("pOut off by 1 byte, float16", setw(pOut=outs[2][1].data_ptr() + 1), "InvalidParameter", f16),
        ("pStream misaligned", lambda j: setattr(j, "pStream", dstream.data_ptr() + 4), "InvalidParameter", f32),
        ("NULL pOut", setw(pOut=None), "ArgumentNull", f32),
        ("NULL pStream", lambda j: setattr(j, "pStream", None), "ArgumentNull", f32),
        ("short stream", lambda j: setattr(j, "streamBytes", 32), "InvalidParameter", f32),
    ]
    for what, bad, code, f in cases:
        assert _name(fn(gpu.ctx, table(bad), 4, C.byref(f), None, s)) == code, what
        untouched(what)
    gpu.check()
    assert fn(gpu.ctx, table(setw(planeStride=7 * 12 + 8)), 4, C.byref(f32), None, s) == 0  # the context is usable afterwards; the smallest plane stride that holds the window
    torch.cuda.synchronize()
    gpu.check()
    assert all(bool((b[:, :, :8] != SENT["float32"]).all()) and bool((b[:, :, 8:] == SENT["float32"]).all()) for b, _ in outs[:2] + outs[3:])
    assert C.sizeof(limg_amd.TensorFormat) == 40 and C.sizeof(Wn) == 7 * C.sizeof(C.c_size_t) and C.sizeof(J) == 11 * C.sizeof(C.c_size_t)


def host_argument_errors(gpu, entry, st):
    """the host form's own: NULL windows / stream / format, count == 0, a bad format, one bad window of three; st: a good stream of an image of at least 64 x 16"""
    ok = np.full((3, 8, 9), SENT["float32"], dtype=np.int32)
    Wn = limg_amd.TensorWindow
    fn = getattr(gpu.lib, entry)
    f32, f16 = fmt_of("float32", 3, "A"), fmt_of("float16", 3, "A")
    good = [Wn(0, 0, 8, 8, ok.ctypes.data, 9, 72), Wn(8, 8, 8, 8, ok.ctypes.data, 9, 72)]
    assert fn(gpu.ctx, st.ctypes.data, st.size, None, 3, C.byref(f32)) == 102 and fn(gpu.ctx, None, st.size, (Wn * 2)(*good), 2, C.byref(f32)) == 102
    assert fn(gpu.ctx, st.ctypes.data, st.size, (Wn * 2)(*good), 2, None) == 102
    assert fn(gpu.ctx, st.ctypes.data, st.size, (Wn * 2)(*good), 0, C.byref(f32)) == 101
    bad_fmt = fmt_of("float32", 3, "A")
    bad_fmt.planes = 5
    assert fn(gpu.ctx, st.ctypes.data, st.size, (Wn * 2)(*good), 2, C.byref(bad_fmt)) == 101
    for bad, code, f in ((Wn(0, 0, 0, 8, ok.ctypes.data, 9, 72), 101, f32), (Wn(0, 0, 8, 8, ok.ctypes.data, 7, 72), 101, f32), (Wn(0, 0, 8, 8, ok.ctypes.data, 9, 70), 101, f32),
                         (Wn(0, 0, 8, 8, ok.ctypes.data + 2, 9, 72), 101, f32), (Wn(0, 0, 8, 8, ok.ctypes.data + 1, 9, 72), 101, f16),
                         (Wn(60, 0, 8, 8, ok.ctypes.data, 9, 72), 103, f32), (Wn(1 << 63, 0, 1 << 63, 1, ok.ctypes.data, 1 << 63, 1 << 63), 103, f32),
                         (Wn(0, 0, 8, 8, None, 9, 72), 102, f32)):
        assert fn(gpu.ctx, st.ctypes.data, st.size, (Wn * 3)(good[0], good[1], bad), 3, C.byref(f)) == code, (bad.x0, bad.width, bad.rowStride, bad.planeStride, code)
        assert (ok == SENT["float32"]).all()
    gpu.check()
