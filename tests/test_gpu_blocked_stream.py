"""GPU parity of version 2 of the compact stream (the merged-block encoder's rectangles): the packer's bytes against the CPU restatement of the container
(oracle/blocked_stream.py, written from the format text in include/limg_hip.h), the GPU decoder and an independent CPU decoder against the pDecoded plane of
the oracle's limg_blocked_encode3d_test, determinism, full-size images through the device entries, context memory, and malformed streams."""
import numpy as np
import pytest

import lib_axis as L
from lib_axis import lib, lib_product  # noqa: F401  (fixtures: "test" / "product")
import limg_amd
from oracle import blocked_stream as B
from blocked_stream_ref import small_cases, stream_flags
from window_cases import ERRORS, SENTINEL

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


def _options(kw):
    return dict(forced_shift=kw.get("forced_shift"), dither_pcg=bool(kw.get("dither_mode", 0)))


def _encode(g, img, alpha, kw):
    g.set_options(**_options(kw))
    try:
        return g.blocked_encode_stream(img, alpha, error_factor=kw.get("error_factor", 100), fast=kw.get("fast", True))
    finally:
        g.set_options()


def _first_diffs(a, b):
    n = min(a.size, b.size)
    return np.argwhere(a[:n] != b[:n])[:8].ravel().tolist()


def test_bytes_roundtrip_and_independent_decode(gpu, oracle):
    saw_escape = False
    for name, img, alpha, kw in small_cases(oracle):
        want = oracle.blocked_encode3d(img, alpha, **kw)
        ref_stream, esc = B.pack(want, img, 4 if alpha else 3, oracle, error_factor=kw.get("error_factor", 100), flags=stream_flags(kw))
        got = _encode(gpu, img, alpha, kw)
        assert got.size == ref_stream.size, (name, got.size, ref_stream.size, _first_diffs(got, ref_stream))
        assert np.array_equal(got, ref_stream), (name, _first_diffs(got, ref_stream))
        saw_escape |= bool((B.parse(got)[1]["shift"] >> 24).any())
        assert esc == 0 or (B.parse(got)[1]["shift"] >> 24).any(), name
        assert len(gpu.blocked_regions()) == len(want["regions"]), name  # limg_hip_blocked_regions keeps working after a stream encode
        assert np.array_equal(gpu.blocked_decode_stream(got), want["pDecoded"]), name  # round trip on the GPU
        assert np.array_equal(B.decode(got, oracle), want["pDecoded"]), name           # the format text, without trusting the GPU decoder
    assert saw_escape


def test_stream_of_the_last_plane_encode(gpu, oracle):
    """limg_hip_blocked_last_stream after a PLANE encode: the same bytes as the stream encode of that image, with no second encode."""
    for img, alpha in ((oracle.random_gradient(203, 61, 5, False), True), (oracle.photo_noise(256, 128, 5), False)):
        h, w = img.shape
        planes = gpu.blocked_encode3d(img, alpha)
        st = gpu.blocked_last_stream(w, h)
        assert np.array_equal(gpu.blocked_decode_stream(st), planes["pDecoded"])
        assert np.array_equal(st, gpu.blocked_encode_stream(img, alpha))
        assert np.array_equal(st, gpu.blocked_last_stream(w, h))


def test_determinism(gpu, lib, oracle):
    other = L.open_context(lib)
    try:
        for img, alpha in ((oracle.photo_noise(256, 128, 5), True), (oracle.random_gradient(203, 61, 5, False), True)):
            a = gpu.blocked_encode_stream(img, alpha)
            assert np.array_equal(a, gpu.blocked_encode_stream(img, alpha))
            assert np.array_equal(a, other.blocked_encode_stream(img, alpha))
        other.check()
    finally:
        other.close()


def _full_size(gpu, kind, n):
    import torch
    img = gpu.synth_device(kind, n, n, seed=1)
    planes = gpu.alloc_blocked_planes_device(n, n)
    gpu.blocked_encode3d_device(img, True, planes)
    torch.cuda.synchronize()
    st, nbytes = gpu.blocked_encode_stream_device(img, True)
    assert 64 < nbytes <= gpu.blocked_stream_bound(n, n)
    regions = gpu.blocked_regions()
    hdr = st[:64].cpu().numpy().view(B.HEADER)[0]
    assert int(hdr["reserved"][0]) == len(regions) and int(hdr["totalBytes"]) == nbytes
    t, k = gpu.blocked_timing(), gpu.blocked_kernel_timing()
    assert t["total"] > 0 and all(v > 0 for v in k.values()), (t, k)
    out = gpu.blocked_decode_stream_device(st, nbytes, n, n)
    torch.cuda.synchronize()
    gpu.check()
    assert torch.equal(out, planes["pDecoded"]), (kind, n)
    return img, nbytes, len(regions)


@pytest.mark.parametrize("kind", ["photo_noise", "random_gradient"])
def test_device_entries_full_size(gpu, oracle, kind):
    n = 2048
    img, nbytes, rects = _full_size(gpu, kind, n)
    himg = img.cpu().numpy().view(np.uint32)
    want = oracle.blocked_encode3d(himg, True, planes=False)
    assert rects == len(want["regions"])
    if kind == "random_gradient":
        blocks = (n // 8) ** 2
        assert len(want["regions"]) < blocks  # a property of the data, checked on the CPU first
        assert rects < blocks
        _, v1 = gpu.encode_stream_device(img, True)
        assert nbytes < v1, (nbytes, v1)  # merging is where the compression comes from


@pytest.mark.parametrize("kind,n", [("random_gradient", 4096), ("photo_noise", 8192)])
def test_device_entries_large(gpu, kind, n):
    _full_size(gpu, kind, n)


def test_context_memory(lib):
    """What the stream encode adds to a context next to the plane encode (device entries, fresh contexts): nothing per pixel -- the factor bytes are packed from the
    encoder's own scratch -- and per block the packer's run prefix (4 bytes, + 1 entry) and per 256 blocks its tile totals (8 bytes); allocations are rounded by the
    driver, hence the slack of a few pages.  The issue's ceiling is 3 B/px + 64 B/block + slack."""
    import torch
    n = 1024
    px, blocks = n * n, (n // 8) ** 2
    a, b = L.open_context(lib), L.open_context(lib)
    try:
        img = a.synth_device("photo_noise", n, n, seed=1)
        a.blocked_encode_stream_device(img, True)
        planes = b.alloc_blocked_planes_device(n, n)
        b.blocked_encode3d_device(img, True, planes)
        torch.cuda.synchronize()
        added = a.device_bytes() - b.device_bytes()
        own = 4 * (blocks + 1) + 8 * ((blocks + 255) // 256)
        print("context bytes: stream encode %d, plane encode %d, added %d (own buffers %d)" % (a.device_bytes(), b.device_bytes(), added, own))
        assert added <= 3 * px + 64 * blocks + 4096
        assert added <= own + 4096
    finally:
        a.close()
        b.close()


def _mutations(oracle, gpu):
    img = oracle.random_gradient(64, 48, 5, False)
    good = gpu.blocked_encode_stream(img, True)
    hdr, table, _ = B.parse(good)
    n = len(table)
    assert n >= 3 and n < 48
    v1 = gpu.encode_stream(img, True)

    def edit(fn):
        s = good.copy()
        fn(s[:64].view(B.HEADER), s[64:64 + 64 * n].view(B.RECT), s)
        return s

    def more_rects(h, t, s):
        h["reserved"][0][0] = 49  # blocks = 48
        h["totalBytes"] = int(h["totalBytes"][0]) + 64 * (49 - n)

    big = int(np.argmax(table["rx"].astype(int) * table["ry"]))
    cases = {
        "wrong magic": edit(lambda h, t, s: h.__setitem__("magic", 0x12345678)),
        "version 1 bytes": v1,
        "truncated table": good[:64 + 64 * (n - 1)],
        "rect outside": edit(lambda h, t, s: t["ox"].__setitem__(n - 1, 8)),
        "payloadWord past the end": edit(lambda h, t, s: t["payloadWord"].__setitem__(n - 1, int(h["payloadWords"][0]) + 1)),
    }
    padded = np.concatenate([good, np.zeros(64 * 64, np.uint8)])
    ph = padded[:64].view(B.HEADER)
    more_rects(ph, None, None)
    cases["R > blocks"] = padded
    # two rectangles overlapping: the second takes the place of the first (which also leaves the second's own blocks uncovered)
    if n >= 2:
        def overlap(h, t, s):
            for f in ("ox", "oy", "rx", "ry"):
                t[f][1] = t[f][0]
        cases["overlap"] = edit(overlap)
    # one block uncovered and nothing else wrong: shrink a rectangle of more than one block by a block row or column
    if table["rx"][big] * table["ry"][big] > 1:
        f = "rx" if table["rx"][big] > 1 else "ry"
        cases["one block uncovered"] = edit(lambda h, t, s: t[f].__setitem__(big, int(t[f][big]) - 1))
    return img, good, v1, cases


def test_malformed_streams_are_refused(gpu, oracle):
    img, good, v1, cases = _mutations(oracle, gpu)
    want = oracle.blocked_encode3d(img, True)["pDecoded"]
    assert {"wrong magic", "version 1 bytes", "truncated table", "R > blocks", "rect outside", "overlap", "one block uncovered", "payloadWord past the end"} <= set(cases)
    for name, s in cases.items():
        with pytest.raises(limg_amd.LimgHipError):
            gpu.blocked_decode_stream(s)
            pytest.fail("accepted: " + name)
        gpu.check()  # reported once
        assert np.array_equal(gpu.blocked_decode_stream(good), want), name  # the context decodes ...
        assert np.array_equal(gpu.blocked_encode_stream(img, True), good), name  # ... and encodes correctly afterwards
    with pytest.raises(limg_amd.LimgHipError):
        gpu.decode_stream(good)  # version 2 bytes given to the version 1 decoder
    assert np.array_equal(gpu.decode_stream(v1), oracle.encode3d(img, True)["pDecoded"])


def test_malformed_streams_on_the_device_entry(gpu, oracle):
    """The kernels' own refusal paths: the device entry does no host-side header check, so every violation is found on the device, pOut is left untouched and
    limg_hip_check_device_status reports it once."""
    import torch
    img, good, v1, cases = _mutations(oracle, gpu)
    h, w = img.shape
    want = oracle.blocked_encode3d(img, True)["pDecoded"]
    for name, s in cases.items():
        if s.size < 64:
            continue
        buf = torch.zeros(good.size + 64 * 64 + 64, dtype=torch.uint8, device="cuda")
        buf[:s.size] = torch.from_numpy(s).cuda()
        out = torch.full((h, w), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        gpu.blocked_decode_stream_device(buf, s.size, w, h, out=out)
        with pytest.raises(limg_amd.LimgHipError):
            gpu.check()
            pytest.fail("accepted: " + name)
        gpu.check()
        assert bool((out == 0x5A5A5A5A).all()), name
        buf[:good.size] = torch.from_numpy(good).cuda()
        got = gpu.blocked_decode_stream_device(buf, good.size, w, h, out=out)
        gpu.check()
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want), name


def test_row_tail_of_half_a_block(gpu, oracle):
    """sizeX % 4 == 0 but sizeX % 8 != 0 (no shape of small_cases has it): the last block column holds 4 pixels while every other column leaves as 16-byte stores.
    Host and device entry against the oracle's pDecoded; the device entry writes nothing beyond the image's last pixel."""
    import torch
    for name, img, alpha in (("pn-12x9", oracle.photo_noise(12, 9, 5), True), ("pn-60x20", oracle.photo_noise(60, 20, 5), True),
                             ("rg-20x8", oracle.random_gradient(20, 8, 5, True), False)):
        h, w = img.shape
        assert w % 4 == 0 and w % 8 != 0
        want = oracle.blocked_encode3d(img, alpha)["pDecoded"]
        st = gpu.blocked_encode_stream(img, alpha)
        assert np.array_equal(gpu.blocked_decode_stream(st), want), name
        out = torch.full((h * w + 16,), SENTINEL, dtype=torch.int32, device="cuda")
        gpu.blocked_decode_stream_device(torch.from_numpy(st).cuda(), st.size, w, h, out=out)
        torch.cuda.synchronize()
        gpu.check()
        got = out.cpu().numpy().view(np.uint32)
        assert np.array_equal(got[:h * w].reshape(h, w), want), name
        assert (got[h * w:] == SENTINEL).all(), name


def test_argument_codes_of_the_device_entry(gpu, oracle):
    """limg_hip_blocked_decode_stream_device's own checks, in its own order: NULL, then geometry and stream size, then the 16-byte alignment of BOTH pointers."""
    import torch
    st = gpu.blocked_encode_stream(oracle.photo_noise(64, 64, 3), True)
    d = torch.from_numpy(st).cuda()
    out = torch.empty((64, 64), dtype=torch.int32, device="cuda")
    fn, s, ps, po = gpu.lib.limg_hip_blocked_decode_stream_device, gpu._stream(), d.data_ptr(), out.data_ptr()
    assert ps % 16 == 0 and po % 16 == 0
    for args, code in (((None, ps, st.size, po, 64, 64), "ArgumentNull"), ((gpu.ctx, None, st.size, po, 64, 64), "ArgumentNull"),
                       ((gpu.ctx, ps, st.size, None, 64, 64), "ArgumentNull"), ((gpu.ctx, ps, st.size, po, 0, 64), "InvalidParameter"),
                       ((gpu.ctx, ps, 32, po, 64, 64), "InvalidParameter"), ((gpu.ctx, ps, st.size, po + 4, 64, 64), "InvalidParameter"),
                       ((gpu.ctx, ps + 8, st.size, po, 64, 64), "InvalidParameter")):
        assert fn(*args, s) == ERRORS[code], (args[1:], code)
    assert fn(gpu.ctx, ps, st.size, po, 64, 64, s) == 0
    torch.cuda.synchronize()
    gpu.check()


L.product_twins(globals())
