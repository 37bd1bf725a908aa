"""limg_hip_encode_stream_batch(_device): a list of same-shape images to version 1 streams in one call -- one compact-mode batched encode, one scan launch
(k_stream_scan_strips_batch: a workgroup per image) and one pack launch (k_stream_pack_strips_batch: waves striding over the strips of all images).  Stream i must be
byte for byte the single call's: against the CPU restatement of the container (oracle/stream.py) at small sizes, against limg_hip_encode_stream(_device) under every
option the batch honours, and on a list long enough that every wave's pipeline crosses images."""
import ctypes as C

import numpy as np
import pytest

import lib_axis as L
from lib_axis import lib, lib_product  # noqa: F401  (fixtures: "test" / "product")
from oracle import stream as S

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


# (name, width, height, images, alpha, encode arguments): seeds and generators of tests/test_gpu_stream.py::_cases, a different seed per image
LISTS = (
    ("one_strip", 256, 8, 3, True, {}),                          # one strip per image: every prefetch of the packer crosses an image
    ("one_block_ef0", 8, 8, 5, True, {"error_factor": 0}),
    ("four_strips", 256, 32, 3, True, {}),                       # imageStrips % 4 == 0: the 16-byte scan path
    ("six_strips_ef400", 264, 24, 5, True, {"error_factor": 400}),  # 2 strips per row, the second of one block; imageStrips % 4 != 0: the dword scan path, slices at 24-byte offsets
    ("rgb", 512, 32, 3, False, {}),
    ("pool", 128, 256, 3, True, {"pool_threads": 2}),
)
SEEDS = (3, 7, 11, 13, 17, 19, 21, 23)


def _images(oracle, w, h, n, first=0):
    """n images: photo-noise and random-gradient (alpha varying) alternate"""
    return [oracle.photo_noise(w, h, SEEDS[(first + i) % len(SEEDS)]) if i % 2 == 0 else oracle.random_gradient(w, h, SEEDS[(first + i) % len(SEEDS)], False) for i in range(n)]


@pytest.fixture(scope="module")
def lists(oracle):
    """every list of LISTS once: its images, the oracle's encode of each and the stream the container's CPU restatement makes of it"""
    out = {}
    for k, (name, w, h, n, alpha, kw) in enumerate(LISTS):
        imgs = _images(oracle, w, h, n, first=k)
        want = [oracle.encode3d(i, alpha, extras=True, **kw) for i in imgs]
        streams = [S.pack(e, w, h, 4 if alpha else 3, error_factor=kw.get("error_factor", 100)) for e in want]
        out[name] = (imgs, alpha, kw, streams, [e["pDecoded"] for e in want])
    return out


def _same(got, want, what):
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.size == b.size, (what, i, a.size, b.size)
        assert np.array_equal(a, b), (what, i, np.argwhere(a != b)[:8].ravel())


def test_bytes_against_the_oracle(gpu, lists):
    saw_escape = False
    for name, (imgs, alpha, kw, streams, decoded) in lists.items():
        got = gpu.encode_stream_batch(imgs, alpha, **kw)
        _same(got, streams, name)
        for st, dec in zip(got, decoded):
            saw_escape |= bool((S.parse(st)[1]["shift"] >> 24).any())
            assert np.array_equal(gpu.decode_stream(st), dec), name
    assert saw_escape


def _singles(gpu, imgs, alpha, **kw):
    return [gpu.encode_stream(i, alpha, **kw) for i in imgs]


def test_batch_equals_single_calls(gpu, lists):
    for name, (imgs, alpha, kw, _, _) in lists.items():
        _same(gpu.encode_stream_batch(imgs, alpha, **kw), _singles(gpu, imgs, alpha, **kw), name)


@pytest.mark.parametrize("sub", [-1, 2, 3])
def test_sub_batches(gpu, oracle, sub):
    """a list of 7 as one launch pair (-1) and as a pipeline of sub-batches of 2 and 3 (the last one short), twice: every sub-batch's payload words, records and shift
    words must land at the list's offsets"""
    for w, h in ((264, 24), (256, 8)):
        imgs = _images(oracle, w, h, 7)
        want = _singles(gpu, imgs, True)
        gpu.set_options(batch_sub_images=sub)
        try:
            for rep in range(2):
                _same(gpu.encode_stream_batch(imgs, True), want, (sub, w, h, rep))
        finally:
            gpu.set_options()


def test_chunks(gpu, oracle):
    """test hook: 3 images per launch pair => 3 + 3 + 1, the last through the single call; with sub-batches inside the chunks too"""
    if not L.has_hooks(gpu):
        return
    imgs = _images(oracle, 264, 24, 7)
    want = _singles(gpu, imgs, True)
    for sub in (0, 2):
        gpu.set_options(test_batch_chunk=3, batch_sub_images=sub)
        try:
            _same(gpu.encode_stream_batch(imgs, True), want, sub)
        finally:
            gpu.set_options()


@pytest.mark.parametrize("opts", [{"forced_shift": (8, 8, 8)}, {"forced_shift": (0, 0, 0)}, {"forced_shift": (7, 8, 1)}, {"dither_pcg": True}, {"float_fast": True}],
                         ids=["shift888", "shift000", "shift781", "pcg", "float_fast"])
def test_options(gpu, oracle, opts):
    """forced_shift, dither_pcg and float_mode = 1 reach the batch as they reach the single call (FAST float mode: against the single FAST encode, not the oracle)"""
    imgs = _images(oracle, 264, 24, 3)
    gpu.set_options(**opts)
    try:
        want = _singles(gpu, imgs, True)
        _same(gpu.encode_stream_batch(imgs, True), want, opts)
    finally:
        gpu.set_options()
    if "float_fast" not in opts and "forced_shift" not in opts:
        plain = _singles(gpu, imgs, True)
        assert any(not np.array_equal(a, b) for a, b in zip(want, plain)), "the option changed nothing: the comparison above shows nothing"


def test_fallbacks(gpu, oracle):
    """images with partial edge blocks, the split path, a list of one: one single-image stream encode per image, the same bytes; an empty list: success"""
    for w, h, n, split in ((203, 61, 3, False), (256, 61, 3, False), (264, 24, 3, True), (264, 24, 1, False)):
        imgs = _images(oracle, w, h, n)
        gpu.set_options(force_split=split)
        try:
            _same(gpu.encode_stream_batch(imgs, True), _singles(gpu, imgs, True), (w, h, n, split))
        finally:
            gpu.set_options()
    assert gpu.encode_stream_batch([], True) == []
    r = gpu.lib.limg_hip_encode_stream_batch_device(gpu.ctx, 0, (C.c_void_p * 1)(), 64, 64, 1, (C.c_void_p * 1)(), gpu.stream_bound(64, 64), None, 100, 0, 1, None)
    assert r == 0


def test_waves_stride_across_images(gpu):
    """520 x 2056: 3 strips per block row, the last of one block, 257 block rows = 771 strips per image (not a multiple of 4); enough images for more than 2 x 16 x CUs
    strips, so that every wave of the packer packs at least two strips with a third in flight and its strips lie in different images.  On the device: every stream
    against the single call's, decode of the first and the last against the plane encode's pDecoded."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    W, H, strips = 520, 2056, 3 * 257
    n = (2 * 16 * cus) // strips + 1
    assert n * strips > 2 * 16 * cus
    imgs = [gpu.synth_device("photo_noise" if i % 2 == 0 else "random_gradient", W, H, seed=1 + i, opaque=False) for i in range(n)]
    outs, sizes = gpu.encode_stream_batch_device(imgs, True)
    for i, img in enumerate(imgs):
        st, nbytes = gpu.encode_stream_device(img, True)
        assert nbytes == sizes[i], (i, nbytes, sizes[i])
        assert torch.equal(st[:nbytes], outs[i][:nbytes]), i
    for i in (0, n - 1):
        planes = gpu.alloc_planes_device(W, H)
        gpu.encode3d_device(imgs[i], True, planes)
        dec = gpu.decode_stream_device(outs[i], sizes[i], W, H)
        torch.cuda.synchronize()
        assert torch.equal(dec, planes["pDecoded"]), i
    gpu.check()


def test_errors(gpu):
    """the contract's refusals, in its order, each before anything touches the device: the output buffers keep their pattern"""
    import torch
    W, H, n = 64, 16, 3
    bound = gpu.stream_bound(W, H)
    imgs = [torch.zeros((H, W), dtype=torch.int32, device="cuda") for _ in range(n)]
    room = torch.full((n, bound + 256), 0x5A, dtype=torch.uint8, device="cuda")
    assert room.data_ptr() % 16 == 0 and (bound + 256) % 16 == 0
    ins = (C.c_void_p * n)(*[i.data_ptr() for i in imgs])
    outs = (C.c_void_p * n)(*[room[i].data_ptr() for i in range(n)])
    sizes = (C.c_size_t * n)()
    dev, host = gpu.lib.limg_hip_encode_stream_batch_device, gpu.lib.limg_hip_encode_stream_batch
    NULL_, INVALID, BOUNDS = 102, 101, 103  # limg_hip_error_ArgumentNull, _InvalidParameter, _OutOfBounds

    def call(ctx=gpu.ctx, count=n, pin=ins, w=W, h=H, pout=outs, cap=bound):
        return dev(ctx, count, pin, w, h, 1, pout, cap, sizes, 100, 0, 1, None)

    assert call(ctx=None) == NULL_
    assert call(pin=None) == NULL_ and call(pout=None) == NULL_
    hole = (C.c_void_p * n)(*[i.data_ptr() for i in imgs]); hole[1] = None
    assert call(pin=hole) == NULL_
    hole = (C.c_void_p * n)(*[room[i].data_ptr() for i in range(n)]); hole[2] = None
    assert call(pout=hole) == NULL_
    assert call(w=0) == INVALID and call(h=0) == INVALID and call(w=1 << 31) == INVALID
    assert call(cap=bound - 1) == BOUNDS
    odd = (C.c_void_p * n)(*[room[i].data_ptr() for i in range(n)]); odd[1] = room[1].data_ptr() + 8  # ppStreams[0] is fine
    assert call(pout=odd) == INVALID
    assert call(w=0, cap=0) == INVALID and call(cap=bound - 1, pout=odd) == BOUNDS  # the order: bound, capacity, alignment
    # the host form: NULL sizes too
    assert host(gpu.ctx, n, ins, W, H, 1, outs, bound, None, 100, 0, 1) == NULL_
    assert host(None, n, ins, W, H, 1, outs, bound, sizes, 100, 0, 1) == NULL_
    torch.cuda.synchronize()
    assert int((room != 0x5A).sum()) == 0, "a refused call wrote to an output buffer"
    assert call() == 0 and all(64 + (W // 8) * (H // 8) * 56 <= s <= bound for s in sizes)  # the context is usable, and the same arguments are accepted
    gpu.check()


def test_back_to_back(gpu, oracle):
    """two batched calls with different lists on one stream, nothing waited for in between: the second must not disturb the first's table, scratch or streams"""
    import torch
    a, b = _images(oracle, 264, 24, 5), _images(oracle, 256, 32, 3, first=2)
    want = [_singles(gpu, a, True), _singles(gpu, b, True)]
    da, db = ([torch.from_numpy(i.view(np.int32)).cuda() for i in l] for l in (a, b))
    torch.cuda.synchronize()
    oa, _ = gpu.encode_stream_batch_device(da, True, want_sizes=False)
    ob, _ = gpu.encode_stream_batch_device(db, True, want_sizes=False)
    torch.cuda.synchronize()
    gpu.check()
    for outs, ref in ((oa, want[0]), (ob, want[1])):
        _same([o[:r.size].cpu().numpy() for o, r in zip(outs, ref)], ref, "back to back")


def test_collect_stats(gpu, oracle):
    """limg_hip_last_stats after a batched stream encode: all images together = the sum of the single encodes' counters"""
    imgs = _images(oracle, 264, 24, 3)
    gpu.set_options(collect_stats=True)
    try:
        total, pixels = np.zeros(30, dtype=np.uint64), 0
        for i in imgs:
            gpu.encode_stream(i, True)
            c, p = gpu.last_stats()
            total += c
            pixels += p
        gpu.encode_stream_batch(imgs, True)
        c, p = gpu.last_stats()
    finally:
        gpu.set_options()
    assert p == pixels == 3 * 264 * 24 and np.array_equal(c, total), (c, total)
    assert int(total[:3].sum()) > 0


def test_context_device_bytes(lib):
    """the factor planes of a chunk -- 3 bytes per pixel per image, where the single call holds one image's -- are context memory the context reports"""
    import torch
    g = L.open_context(lib)
    try:
        W, H, n = 512, 256, 4
        imgs = [g.synth_device("photo_noise", W, H, seed=1 + i) for i in range(n)]
        outs = [torch.empty(g.stream_bound(W, H), dtype=torch.uint8, device="cuda") for _ in range(n)]
        g.encode_stream_device(imgs[0], True, out=outs[0])
        before = g.device_bytes()
        g.encode_stream_batch_device(imgs, True, outs=outs)
        assert g.device_bytes() - before >= 3 * W * H * (n - 1), (before, g.device_bytes())
        fresh = L.open_context(lib)
        try:
            base = fresh.device_bytes()
            fresh.encode_stream_batch_device(imgs, True, outs=outs)
            assert fresh.device_bytes() - base >= 3 * W * H * n
            fresh.check()
        finally:
            fresh.close()
        g.check()
    finally:
        g.close()


L.product_twins(globals())  # test_x_product: the same tests on the product library (tests/lib_axis.py)
