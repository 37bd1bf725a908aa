"""What the GPU tests of the error windows of both stream versions share (tests/test_gpu_stream_error.py, tests/test_gpu_blocked_stream_error.py): the images, the
windows, the two originals in their two placements, one batched call checked against the numpy restatement (tests/stream_error_ref.py) on the oracle's decode, and the
host refusals.  `V`: what differs between the versions -- the entries' names and the oracle's decode.  Not a test module."""
import ctypes as C

import numpy as np

import limg_amd
from stream_error_ref import error_sum
from window_batch import device_stream
from window_cases import ERRORS, SENTINEL

SUM_SENTINEL = 0x5A5A5A5A5A5A5A5A

# name, width, height, alpha, generator.  536 = 67 blocks: version 1 has two units per block row, the second of 3 blocks; version 2 nine, the last of 3.
SHAPES = (("8x8", 8, 8, True, "photo_noise", 3), ("536x24", 536, 24, True, "gradient_alpha", 7), ("520x16_rgb", 520, 16, False, "photo_noise", 11),
          ("75x21", 75, 21, True, "gradient_alpha", 13))


class Version:
    def __init__(self, blocked):
        self.blocked = blocked
        self.prefix = "blocked_" if blocked else ""
        self.symbol = "limg_hip_%sdecode_stream_windows_error" % self.prefix

    def encode(self, gpu, img, alpha):
        return (gpu.blocked_encode_stream if self.blocked else gpu.encode_stream)(img, alpha)

    def decoded(self, oracle, img, alpha):
        return (oracle.blocked_encode3d if self.blocked else oracle.encode3d)(img, alpha)["pDecoded"]

    def device(self, gpu):
        return getattr(gpu, self.prefix + "decode_stream_windows_error_device")

    def host(self, gpu):
        return getattr(gpu, self.prefix + "decode_stream_windows_error")


_REF = {}


def images(oracle, V):
    """{name: (img, alpha, channels, the oracle's decode)}: computed once per version, shared, never changed"""
    if V.blocked not in _REF:
        out = {}
        for name, w, h, alpha, kind, seed in SHAPES:
            img = oracle.photo_noise(w, h, seed) if kind == "photo_noise" else oracle.random_gradient(w, h, seed, False)
            out[name] = (img, alpha, 4 if alpha else 3, V.decoded(oracle, img, alpha))
        _REF[V.blocked] = out
    return _REF[V.blocked]


def windows(w, h):
    """the whole image; (3, 5, w - 7, h - 9); the last pixel alone; a one-pixel column of full height at x0 = 7; x 505 .. 530 of the 536-wide image: across the boundary
    between two 64-block units of version 1 (block 64 starts at x = 512) and between version 2's units 7 and 8 (x = 512 as well)"""
    wins = [(0, 0, w, h), (w - 1, h - 1, 1, 1), (7, 0, 1, h)]
    if w > 7 and h > 9:
        wins.append((3, 5, w - 7, h - 9))
    if w == 536:
        wins.append((505, 0, 26, h))
    return wins


def random_original(w, h, seed):
    return np.random.default_rng(seed).integers(0, 2 ** 32, (h, w), dtype=np.uint32)


class Layout:
    """Originals on the device: add() a window's crop densely (a tensor of its own, 16-byte aligned, stride = width) or at a stride of width + 3 from a pointer that is
    4-byte but not 16-byte aligned, inside a sentinel-filled tensor.  untouched(): every tensor still holds what it was given."""

    def __init__(self):
        self.kept = []

    def add(self, crop, strided):
        import torch
        h, w = crop.shape
        if not strided:
            t = torch.from_numpy(np.ascontiguousarray(crop).view(np.int32)).cuda()
            assert t.data_ptr() % 16 == 0
            self.kept.append((t, t.clone()))
            return t, w
        stride = w + 3
        flat = torch.full((1 + h * stride + 4,), SENTINEL, dtype=torch.int32, device="cuda")
        flat[1:1 + h * stride].view(h, stride)[:, :w] = torch.from_numpy(np.ascontiguousarray(crop).view(np.int32)).cuda()
        assert flat.data_ptr() % 16 == 0 and flat[1:].data_ptr() % 16 == 4
        self.kept.append((flat, flat.clone()))
        return flat[1:], stride

    def untouched(self):
        import torch
        return all(torch.equal(a, b) for a, b in self.kept)


def sums_tensor(n):
    """n sums inside a sentinel-filled tensor -> (the whole tensor, its slice for the call)"""
    import torch
    big = torch.full((n + 4,), SUM_SENTINEL, dtype=torch.int64, device="cuda")
    return big, big[2:2 + n]


def jobs_of(V, gpu, oracle, name, layout, first_seed=100):
    """every window x {the encoded image, a random image} x {dense, strided} of one shape -> (job tuples of the device entry, expected sums)"""
    img, alpha, channels, dec = images(oracle, V)[name]
    h, w = img.shape
    st = V.encode(gpu, img, alpha)
    d = device_stream(st)
    jobs, want = [], []
    for k, win in enumerate(windows(w, h)):
        x, y, ww, hh = win
        for original in (img, random_original(w, h, first_seed + k)):
            for strided in (False, True):
                t, stride = layout.add(original[y:y + hh, x:x + ww], strided)
                jobs.append((d, st.size, w, h, x, y, ww, hh, t, stride))
                want.append(error_sum(dec, original, channels, win))
    return jobs, want


def run(V, gpu, jobs, want, layout, ctx):
    """one batched call: every sum is the expected one, the status words are 0, nothing around the sums and no original has changed"""
    import torch
    big, sums = sums_tensor(len(jobs))
    status = torch.full((len(jobs),), 77, dtype=torch.int32, device="cuda")
    V.device(gpu)(jobs, sums=sums, status=status)
    torch.cuda.synchronize()
    got = sums.cpu().tolist()
    print(ctx, got[:8], want[:8])
    assert got == want, (ctx, [(i, g, w_) for i, (g, w_) in enumerate(zip(got, want)) if g != w_][:6])
    assert big[:2].cpu().tolist() == [SUM_SENTINEL] * 2 and big[-2:].cpu().tolist() == [SUM_SENTINEL] * 2, ctx
    assert not bool(status.any()), (ctx, status.cpu().tolist())
    assert layout.untouched(), ctx
    gpu.check()
    return got


def _name(r):
    return {v: k for k, v in ERRORS.items()}.get(r, r)


def host_refusals(V, gpu, dstream, nbytes, W, H):
    """the device entry's refusals on the host: the documented codes, with a sentinel-filled sums array untouched.  dstream: a good stream of a W x H image, W, H >= 16"""
    import torch
    fn = getattr(gpu.lib, V.symbol + "_device")
    s = gpu._stream()
    originals = [torch.zeros((8, 12), dtype=torch.int32, device="cuda") for _ in range(4)]
    big, sums = sums_tensor(4)
    ps = C.c_void_p(sums.data_ptr())

    def table(bad=None):
        t = (limg_amd.ErrorWindowJob * 4)()
        for i in range(4):
            t[i] = limg_amd.ErrorWindowJob(dstream.data_ptr(), nbytes, W, H, limg_amd.ErrorWindow(8 * (i % 2), 0, 8, 8, originals[i].data_ptr(), 12))
        if bad:
            bad(t[2])
        return t

    def setw(**kw):
        def f(j):
            for k, v in kw.items():
                setattr(j.window, k, v)
        return f

    assert _name(fn(gpu.ctx, table(), 0, ps, None, s)) == "InvalidParameter"
    assert _name(fn(gpu.ctx, None, 4, ps, None, s)) == "ArgumentNull"
    assert _name(fn(None, table(), 4, ps, None, s)) == "ArgumentNull"
    assert _name(fn(gpu.ctx, table(), 4, None, None, s)) == "ArgumentNull"
    cases = [
        ("NULL pOriginal", setw(pOriginal=None), "ArgumentNull"),
        ("NULL pStream", lambda j: setattr(j, "pStream", None), "ArgumentNull"),
        ("zero width", setw(width=0), "InvalidParameter"),
        ("stride < width", setw(originalStridePixels=7), "InvalidParameter"),
        ("pOriginal misaligned by 2", setw(pOriginal=originals[2].data_ptr() + 2), "InvalidParameter"),
        ("pStream misaligned", lambda j: setattr(j, "pStream", dstream.data_ptr() + 4), "InvalidParameter"),
        ("window outside the image", setw(x0=W - 4), "OutOfBounds"),
        ("below the image", setw(y0=H), "OutOfBounds"),
        ("overflow", setw(x0=1 << 63, width=1 << 63, originalStridePixels=1 << 63), "OutOfBounds"),
    ]
    for what, bad, code in cases:
        assert _name(fn(gpu.ctx, table(bad), 4, ps, None, s)) == code, what
        torch.cuda.synchronize()
        assert big.cpu().tolist() == [SUM_SENTINEL] * 8, what
    gpu.check()
    assert fn(gpu.ctx, table(), 4, ps, None, s) == 0  # the context is usable afterwards, and the good list is measured
    torch.cuda.synchronize()
    gpu.check()
    got = sums.cpu().tolist()
    assert got[0] == got[2] and got[1] == got[3] and SUM_SENTINEL not in got and big[:2].cpu().tolist() == [SUM_SENTINEL] * 2
    assert C.sizeof(limg_amd.ErrorWindow) == 6 * C.sizeof(C.c_size_t) and C.sizeof(limg_amd.ErrorWindowJob) == 10 * C.sizeof(C.c_size_t)


def host_form_refusals(V, gpu, st, W, H):
    """the host form's own refusals: NULL stream / windows / sums, count == 0, one bad window of three, a stream refused on the device -- the sums keep their sentinel"""
    fn = getattr(gpu.lib, V.symbol)
    o = np.zeros((8, 9), dtype=np.uint32)
    sums = (C.c_uint64 * 5)(*([SUM_SENTINEL] * 5))
    E = limg_amd.ErrorWindow
    good = [E(0, 0, 8, 8, o.ctypes.data, 9), E(8, 8, 8, 8, o.ctypes.data, 9)]
    assert _name(fn(gpu.ctx, st.ctypes.data, st.size, None, 2, sums)) == "ArgumentNull" and _name(fn(gpu.ctx, None, st.size, (E * 2)(*good), 2, sums)) == "ArgumentNull"
    assert _name(fn(gpu.ctx, st.ctypes.data, st.size, (E * 2)(*good), 2, None)) == "ArgumentNull" and _name(fn(None, st.ctypes.data, st.size, (E * 2)(*good), 2, sums)) == "ArgumentNull"
    assert _name(fn(gpu.ctx, st.ctypes.data, st.size, (E * 2)(*good), 0, sums)) == "InvalidParameter"
    for bad, code in ((E(0, 0, 0, 8, o.ctypes.data, 9), "InvalidParameter"), (E(0, 0, 8, 8, o.ctypes.data, 7), "InvalidParameter"), (E(W - 4, 0, 8, 8, o.ctypes.data, 9), "OutOfBounds"),
                      (E(0, H, 8, 1, o.ctypes.data, 9), "OutOfBounds"), (E(0, 0, 8, 8, None, 9), "ArgumentNull")):
        assert _name(fn(gpu.ctx, st.ctypes.data, st.size, (E * 3)(good[0], good[1], bad), 3, sums)) == code, (bad.x0, bad.width, code)
    assert _name(fn(gpu.ctx, st.ctypes.data, st.size - 8, (E * 2)(*good), 2, sums)) == "OutOfBounds"  # shorter than its header says
    bad_magic = st.copy()
    bad_magic[0] ^= 0xFF
    assert fn(gpu.ctx, bad_magic.ctypes.data, st.size, (E * 2)(*good), 2, sums) != 0
    assert list(sums) == [SUM_SENTINEL] * 5
    gpu.check()
    assert fn(gpu.ctx, st.ctypes.data, st.size, (E * 2)(*good), 2, sums) == 0 and list(sums)[2:] == [SUM_SENTINEL] * 3 and SUM_SENTINEL not in list(sums)[:2]
    gpu.check()
