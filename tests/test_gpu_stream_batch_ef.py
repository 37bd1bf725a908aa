"""limg_hip_encode_stream_batch_ef(_device): a list of same-shape images to version 1 streams in one call, image i at its own error factor -- one float-stage grid,
one persistent launch of k_encode_list_rated (the thresholds per work strip from a device table), one scan (which writes every header's own error factor) and one
pack.  Stream i must be byte for byte the single call's at error_factors[i]: against the CPU restatement of the container (oracle/stream.py), against
limg_hip_encode_stream(_device) under every option the batch honours, on lists longer than one table launch, in sub-batches and chunks, and through the fallbacks.
The budgeted list's final encodes take the same route: one encode per chunk whatever its searches chose."""
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


# (name, width, height, alpha, error factors -- one image each --, encode arguments)
LISTS = (
    ("six_strips", 264, 24, True, (0, 1, 2, 101, 400), {}),   # images without crush bits beside crushed ones; imageStrips % 4 != 0: the dword scan path
    ("one_strip", 256, 8, True, (400, 0, 50), {}),            # one strip per image: every workgroup's F step belongs to another image than its E step
    ("one_block", 8, 8, True, (3, 40, 0, 1000, 128), {}),
    ("rgb", 512, 32, False, (20, 300, 100), {}),
    ("pool", 128, 256, True, (60, 7, 250), {"pool_threads": 2}),
    ("four_strips", 256, 32, True, (10, 200, 64), {}),        # imageStrips % 4 == 0: the 16-byte scan path
)
SEEDS = (3, 7, 11, 13, 17, 19, 21, 23)
SEVEN = (2, 400, 0, 37, 100, 1, 256)


def _images(oracle, w, h, n, first=0):
    """n images: photo-noise and random-gradient (alpha varying) alternate"""
    return [oracle.photo_noise(w, h, SEEDS[(first + i) % len(SEEDS)]) if i % 2 == 0 else oracle.random_gradient(w, h, SEEDS[(first + i) % len(SEEDS)], False) for i in range(n)]


@pytest.fixture(scope="module")
def lists(oracle):
    """every list of LISTS once: its images, the stream the container's CPU restatement makes of the oracle's encode of image i at factor i, and that encode's pDecoded"""
    out = {}
    for k, (name, w, h, alpha, efs, kw) in enumerate(LISTS):
        imgs = _images(oracle, w, h, len(efs), first=k)
        want = [oracle.encode3d(i, alpha, extras=True, error_factor=ef, **kw) for i, ef in zip(imgs, efs)]
        streams = [S.pack(e, w, h, 4 if alpha else 3, error_factor=ef) for e, ef in zip(want, efs)]
        out[name] = (imgs, alpha, efs, kw, streams, [e["pDecoded"] for e in want])
    return out


def _same(got, want, what):
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.size == b.size, (what, i, a.size, b.size)
        assert np.array_equal(a, b), (what, i, np.argwhere(a != b)[:8].ravel())


def _singles(gpu, imgs, alpha, efs, **kw):
    return [gpu.encode_stream(i, alpha, error_factor=ef, **kw) for i, ef in zip(imgs, efs)]


def test_bytes_against_the_oracle(gpu, lists):
    for name, (imgs, alpha, efs, kw, streams, decoded) in lists.items():
        got = gpu.encode_stream_batch_ef(imgs, alpha, efs, **kw)
        _same(got, streams, name)
        for st, dec, ef in zip(got, decoded, efs):
            assert int(S.parse(st)[0]["errorFactor"]) == ef, (name, ef)
            assert np.array_equal(gpu.decode_stream(st), dec), name


def test_equals_single_calls(gpu, lists):
    for name, (imgs, alpha, efs, kw, _, _) in lists.items():
        _same(gpu.encode_stream_batch_ef(imgs, alpha, efs, **kw), _singles(gpu, imgs, alpha, efs, **kw), name)


def test_equals_the_shared_factor_batch(gpu, lists):
    for name, (imgs, alpha, efs, kw, _, _) in lists.items():
        ef = efs[0]
        _same(gpu.encode_stream_batch_ef(imgs, alpha, [ef] * len(imgs), **kw), gpu.encode_stream_batch(imgs, alpha, error_factor=ef, **kw), (name, ef))


def test_table_longer_than_one_launch(gpu, oracle):
    """66 images of one block: more than one launch of the threshold table carries (64)"""
    base = _images(oracle, 8, 8, 8)
    imgs = [base[i % 8] for i in range(66)]
    efs = [SEVEN[i % 7] for i in range(66)]
    memo = {}
    want = []
    for i in range(66):
        key = (i % 8, efs[i])
        if key not in memo:
            memo[key] = gpu.encode_stream(imgs[i], True, error_factor=efs[i])
        want.append(memo[key])
    _same(gpu.encode_stream_batch_ef(imgs, True, efs), want, "66")


@pytest.mark.parametrize("sub", [-1, 2, 3])
def test_sub_batches(gpu, oracle, sub):
    """a list of 7 at seven factors as one launch pair (-1) and as a pipeline of sub-batches of 2 and 3 (the last one short), twice: every sub-batch numbers its strips
    and its images from 0, so its slice of the threshold table must be offset as its records are"""
    for w, h in ((264, 24), (256, 8)):
        imgs = _images(oracle, w, h, 7)
        want = _singles(gpu, imgs, True, SEVEN)
        gpu.set_options(batch_sub_images=sub)
        try:
            for rep in range(2):
                _same(gpu.encode_stream_batch_ef(imgs, True, SEVEN), want, (sub, w, h, rep))
        finally:
            gpu.set_options()


def test_chunks(gpu, oracle):
    """test hook: 3 images per launch pair => 3 + 3 + 1, the last through the single call; with sub-batches inside the chunks too"""
    if not L.has_hooks(gpu):
        return
    imgs = _images(oracle, 264, 24, 7)
    want = _singles(gpu, imgs, True, SEVEN)
    for sub in (0, 2):
        gpu.set_options(test_batch_chunk=3, batch_sub_images=sub)
        try:
            _same(gpu.encode_stream_batch_ef(imgs, True, SEVEN), want, sub)
        finally:
            gpu.set_options()


@pytest.mark.parametrize("opts", [{"forced_shift": (8, 8, 8)}, {"forced_shift": (0, 0, 0)}, {"forced_shift": (7, 8, 1)}, {"dither_pcg": True}, {"float_fast": True}],
                         ids=["shift888", "shift000", "shift781", "pcg", "float_fast"])
def test_options(gpu, oracle, opts):
    """forced_shift, dither_pcg and float_mode = 1 reach the list as they reach the single call; under a forced shift the streams of one image at two factors differ in
    the header's error factor only"""
    imgs = _images(oracle, 264, 24, 3)
    efs = (2, 100, 400)
    gpu.set_options(**opts)
    try:
        want = _singles(gpu, imgs, True, efs)
        got = gpu.encode_stream_batch_ef(imgs, True, efs)
        _same(got, want, opts)
        if "forced_shift" in opts:
            again = gpu.encode_stream_batch_ef(imgs, True, (400, 2, 100))
            for a, b, ea, eb in zip(got, again, efs, (400, 2, 100)):
                ha, hb = S.parse(a)[0], S.parse(b)[0]
                assert int(ha["errorFactor"]) == ea and int(hb["errorFactor"]) == eb
                differ = np.flatnonzero(a != b)
                field = S.HEADER.fields["errorFactor"][1]
                assert a.size == b.size and differ.size > 0 and differ.min() >= field and differ.max() < field + 4, (opts, differ[:8])
    finally:
        gpu.set_options()
    if "dither_pcg" in opts:
        plain = _singles(gpu, imgs, True, efs)
        assert any(not np.array_equal(a, b) for a, b in zip(want, plain)), "the option changed nothing: the comparison above shows nothing"


def test_generic_search(gpu, oracle):
    """test hook record_limit lowered: every block takes the generic 32-bit search, whose block limit is the per-image maxBlock"""
    if not L.has_hooks(gpu):
        return
    imgs = _images(oracle, 264, 24, 3)
    efs = (2, 100, 400)
    plain = _singles(gpu, imgs, True, efs)
    gpu.set_options(test_record_limit=1)
    try:
        want = _singles(gpu, imgs, True, efs)
        _same(gpu.encode_stream_batch_ef(imgs, True, efs), want, "record_limit")
    finally:
        gpu.set_options()
    _same(want, plain, "the generic search is exact")


def test_fallbacks(gpu, oracle):
    """images with partial edge blocks, the split path, a list of one, the accurate search: the existing entries, grouped by error factor, the same bytes; an empty
    list: success"""
    for w, h, n, split, fast in ((203, 61, 3, False, True), (256, 61, 3, False, True), (264, 24, 3, True, True), (264, 24, 1, False, True), (264, 24, 4, False, False)):
        imgs = _images(oracle, w, h, n)
        efs = (100, 30, 100, 30)[:n] if not fast else (30, 400, 7)[:n]
        gpu.set_options(force_split=split)
        try:
            _same(gpu.encode_stream_batch_ef(imgs, True, efs, fast=fast), _singles(gpu, imgs, True, efs, fast=fast), (w, h, n, split, fast))
        finally:
            gpu.set_options()
    assert gpu.encode_stream_batch_ef([], True, []) == []
    r = gpu.lib.limg_hip_encode_stream_batch_ef_device(gpu.ctx, 0, (C.c_void_p * 1)(), 64, 64, 1, (C.c_void_p * 1)(), gpu.stream_bound(64, 64), None, (C.c_uint32 * 1)(), 0, 1,
                                                       None)
    assert r == 0


def test_waves_stride_across_images(gpu):
    """the 520 x 2056 list of tests/test_gpu_stream_batch.py, factors alternating 50 / 200, on the device: every stream against the single call's"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    W, H, strips = 520, 2056, 3 * 257
    n = (2 * 16 * cus) // strips + 1
    assert n * strips > 2 * 16 * cus
    imgs = [gpu.synth_device("photo_noise" if i % 2 == 0 else "random_gradient", W, H, seed=1 + i, opaque=False) for i in range(n)]
    efs = [50 if i % 2 == 0 else 200 for i in range(n)]
    outs, sizes = gpu.encode_stream_batch_ef_device(imgs, True, efs)
    for i, img in enumerate(imgs):
        st, nbytes = gpu.encode_stream_device(img, True, error_factor=efs[i])
        assert nbytes == sizes[i], (i, nbytes, sizes[i])
        assert torch.equal(st[:nbytes], outs[i][:nbytes]), i
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
    factors = (C.c_uint32 * n)(0, 100, 401)
    dev, host = gpu.lib.limg_hip_encode_stream_batch_ef_device, gpu.lib.limg_hip_encode_stream_batch_ef
    NULL_, INVALID, BOUNDS = 102, 101, 103  # limg_hip_error_ArgumentNull, _InvalidParameter, _OutOfBounds

    def call(ctx=gpu.ctx, count=n, pin=ins, w=W, h=H, pout=outs, cap=bound, efs=factors):
        return dev(ctx, count, pin, w, h, 1, pout, cap, sizes, efs, 0, 1, None)

    assert call(ctx=None) == NULL_
    assert call(pin=None) == NULL_ and call(pout=None) == NULL_ and call(efs=None) == NULL_
    assert call(efs=None, count=0) == NULL_ and call(efs=None, w=0) == NULL_  # a pointer: before the shape and before the empty list
    hole = (C.c_void_p * n)(*[i.data_ptr() for i in imgs]); hole[1] = None
    assert call(pin=hole) == NULL_
    hole = (C.c_void_p * n)(*[room[i].data_ptr() for i in range(n)]); hole[2] = None
    assert call(pout=hole) == NULL_
    assert call(w=0) == INVALID and call(h=0) == INVALID and call(w=1 << 31) == INVALID
    assert call(cap=bound - 1) == BOUNDS
    odd = (C.c_void_p * n)(*[room[i].data_ptr() for i in range(n)]); odd[1] = room[1].data_ptr() + 8  # ppStreams[0] is fine
    assert call(pout=odd) == INVALID
    assert call(w=0, cap=0) == INVALID and call(cap=bound - 1, pout=odd) == BOUNDS  # the order: bound, capacity, alignment
    # the host form: NULL sizes and NULL factors too
    assert host(gpu.ctx, n, ins, W, H, 1, outs, bound, None, factors, 0, 1) == NULL_
    assert host(gpu.ctx, n, ins, W, H, 1, outs, bound, sizes, None, 0, 1) == NULL_
    assert host(None, n, ins, W, H, 1, outs, bound, sizes, factors, 0, 1) == NULL_
    torch.cuda.synchronize()
    assert int((room != 0x5A).sum()) == 0, "a refused call wrote to an output buffer"
    assert call() == 0 and all(64 + (W // 8) * (H // 8) * 56 <= s <= bound for s in sizes)  # the context is usable, and the same arguments are accepted
    torch.cuda.synchronize()
    assert [int(room[i][:64].cpu().numpy().view(S.HEADER)[0]["errorFactor"]) for i in range(n)] == [0, 100, 401]
    gpu.check()


def test_back_to_back(gpu, oracle):
    """two calls with different lists and factor tables on one stream, nothing waited for in between: the second must not disturb the first's tables, scratch or streams"""
    import torch
    a, b = _images(oracle, 264, 24, 5), _images(oracle, 256, 32, 3, first=2)
    ea, eb = (400, 2, 100, 0, 31), (5, 300, 64)
    want = [_singles(gpu, a, True, ea), _singles(gpu, b, True, eb)]
    da, db = ([torch.from_numpy(i.view(np.int32)).cuda() for i in l] for l in (a, b))
    torch.cuda.synchronize()
    oa, _ = gpu.encode_stream_batch_ef_device(da, True, ea, want_sizes=False)
    ob, _ = gpu.encode_stream_batch_ef_device(db, True, eb, want_sizes=False)
    torch.cuda.synchronize()
    gpu.check()
    for outs, ref in ((oa, want[0]), (ob, want[1])):
        _same([o[:r.size].cpu().numpy() for o, r in zip(outs, ref)], ref, "back to back")


def _summed_stats(gpu, imgs, efs):
    total, pixels = np.zeros(30, dtype=np.uint64), 0
    for i, ef in zip(imgs, efs):
        gpu.encode_stream(i, True, error_factor=ef)
        c, p = gpu.last_stats()
        total += c
        pixels += p
    return total, pixels


def test_collect_stats(gpu, oracle):
    """limg_hip_last_stats after the call: all images together = the sum of the single encodes' counters at their factors"""
    imgs = _images(oracle, 264, 24, 3)
    efs = (2, 100, 400)
    gpu.set_options(collect_stats=True)
    try:
        total, pixels = _summed_stats(gpu, imgs, efs)
        gpu.encode_stream_batch_ef(imgs, True, efs)
        c, p = gpu.last_stats()
    finally:
        gpu.set_options()
    assert p == pixels == 3 * 264 * 24 and np.array_equal(c, total), (c, total)
    assert int(total[:3].sum()) > 0


def test_budgeted_list_is_one_encode(gpu, oracle):
    """limg_hip_encode_stream_budget_batch: after the searches the chunk is ONE encode at the chosen factors -- limg_hip_last_stats then covers all five images (on
    the grouped route it covered the last group only); results and streams are those of the loop of single budget calls"""
    W, H = 264, 24
    imgs = [oracle.photo_noise(W, H, 3), oracle.random_gradient(W, H, 7, False), oracle.photo_noise(W, H, 11), oracle.random_gradient(W, H, 13, True), oracle.photo_noise(W, H, 17)]
    gpu.set_options(collect_stats=True)
    try:
        streams, results = gpu.encode_stream_budget_batch(imgs, True, 11500, 2, 128)
        c, p = gpu.last_stats()
        efs = [r.errorFactor for r in results]
        assert len(set(efs)) >= 2, efs
        total, pixels = _summed_stats(gpu, imgs, efs)
        assert p == pixels == 5 * W * H and np.array_equal(c, total), (p, c, total)
        for i, img in enumerate(imgs):
            one_st, one = gpu.encode_stream_budget(img, True, 11500, 2, 128)
            assert (results[i].errorFactor, results[i].withinBudget, results[i].probes, results[i].bytes) == (one.errorFactor, one.withinBudget, one.probes, one.bytes), i
            assert np.array_equal(streams[i], one_st), i
    finally:
        gpu.set_options()


L.product_twins(globals())  # test_x_product: the same tests on the product library (tests/lib_axis.py)
