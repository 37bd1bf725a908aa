"""limg_hip_encode_stream_quality_list(_device): a list of images of MIXED shapes, each to its own quality target.  pResults[i] and stream i must be exactly
limg_hip_encode_stream_quality's for item i alone -- the rounds' encodes go through limg_hip_encode_stream_list_device, the error launch takes jobs of any shape --
and the refusals come before anything touches the device."""
import ctypes as C

import numpy as np
import pytest

import lib_axis as L
from lib_axis import lib, lib_product  # noqa: F401  (fixtures: "test" / "product")
from limg_amd import QualityResult, StreamListItem

pytestmark = pytest.mark.gpu

EDGES = ((264, 24), (8, 8), (256, 8), (520, 16), (8, 512), (24, 40), (512, 32))
POOL = ((128, 256), (64, 24), (8, 8), (256, 40))
FIELDS = ("errorFactor", "probes", "withinTarget", "bytes", "errorSum")


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


def _images(oracle, shapes):
    return [oracle.photo_noise(w, h, 3 + 2 * (i % 8)) if i % 2 == 0 else oracle.random_gradient(w, h, 3 + 2 * (i % 8), False) for i, (w, h) in enumerate(shapes)]


def _limits(gpu, shapes):
    """two PSNR targets and one limit of 0 (lossless), cycling through the list"""
    return [0 if i % 3 == 2 else gpu.error_sum_for_psnr(w, h, True, (34.0, 42.0)[i % 3]) for i, (w, h) in enumerate(shapes)]


@pytest.mark.parametrize("name,shapes,kw", [("edges", EDGES, {}), ("pool", POOL, {"pool_threads": 2})], ids=["edges", "pool"])
def test_results_and_streams_are_the_single_calls(gpu, oracle, name, shapes, kw):
    imgs = _images(oracle, shapes)
    limits = _limits(gpu, shapes)
    streams, results = gpu.encode_stream_quality_list(imgs, True, limits, **kw)
    assert len({r.errorFactor for r in results}) >= 2, "every search chose the same factor: the list shows little"
    for i, (img, lim) in enumerate(zip(imgs, limits)):
        st, one = gpu.encode_stream_quality(img, True, lim, **kw)
        assert tuple(getattr(results[i], f) for f in FIELDS) == tuple(getattr(one, f) for f in FIELDS), (name, i)
        assert np.array_equal(streams[i], st), (name, i)
    # the device form
    import torch
    dimgs = [torch.from_numpy(i.view(np.int32)).cuda() for i in imgs]
    outs, dres = gpu.encode_stream_quality_list_device(dimgs, True, limits, **kw)
    torch.cuda.synchronize()
    for i in range(len(imgs)):
        assert tuple(getattr(dres[i], f) for f in FIELDS) == tuple(getattr(results[i], f) for f in FIELDS), (name, i)
        assert np.array_equal(outs[i][:dres[i].bytes].cpu().numpy(), streams[i]), (name, i)
    gpu.check()


def test_min_psnr_goes_through_error_sum_for_psnr(gpu, oracle):
    shapes = EDGES[:3]
    imgs = _images(oracle, shapes)
    a, ra = gpu.encode_stream_quality_list(imgs, True, min_psnr=38.0)
    b, rb = gpu.encode_stream_quality_list(imgs, True, [gpu.error_sum_for_psnr(w, h, True, 38.0) for w, h in shapes])
    assert [r.errorFactor for r in ra] == [r.errorFactor for r in rb] and all(np.array_equal(x, y) for x, y in zip(a, b))


def test_errors(gpu):
    """the list encode's refusals, then the search's bound rules and struct_size, then the empty list: canary-filled stream buffers and results stay untouched"""
    import torch
    shapes = ((64, 16), (8, 8), (264, 24))
    n = len(shapes)
    imgs = [torch.zeros((h, w), dtype=torch.int32, device="cuda") for w, h in shapes]
    bounds = [gpu.stream_bound(w, h) for w, h in shapes]
    room = [torch.full((b,), 0x5A, dtype=torch.uint8, device="cuda") for b in bounds]
    limits = (C.c_uint64 * n)(1000, 0, 5000)
    dev, host = gpu.lib.limg_hip_encode_stream_quality_list_device, gpu.lib.limg_hip_encode_stream_quality_list
    NULL_, INVALID, BOUNDS = 102, 101, 103
    SIZE = C.sizeof(StreamListItem)

    def items(**change):
        it = (StreamListItem * n)()
        for k in range(n):
            it[k] = StreamListItem(imgs[k].data_ptr(), room[k].data_ptr(), bounds[k], shapes[k][0], shapes[k][1], 0xDEAD, 0)  # (errorFactor is ignored)
        for name, v in change.items():
            setattr(it[1], name, v)
        return it

    def results(size=C.sizeof(QualityResult)):
        res = (QualityResult * n)()
        for r in res:
            r.struct_size, r.errorFactor, r.bytes = size, 0x5A5A, 0x5A5A
        return res

    res = results()

    def call(ctx=gpu.ctx, count=n, it=None, size=SIZE, lim=limits, lo=0, hi=0, out=res):
        return dev(ctx, count, items() if it is None else it, size, 1, lim, lo, hi, 0, 1, out, None)

    assert call(ctx=None) == NULL_ and call(lim=None) == NULL_ and call(out=None) == NULL_ and dev(gpu.ctx, n, None, SIZE, 1, limits, 0, 0, 0, 1, res, None) == NULL_
    assert call(out=None, count=0) == NULL_ and call(lim=None, size=0) == NULL_  # the pointers: before the item size and before the empty list
    assert call(size=SIZE - 1) == INVALID
    assert call(it=items(pStream=None)) == NULL_ and call(it=items(sizeY=0)) == INVALID and call(it=items(pStream=room[1].data_ptr() + 8)) == INVALID
    assert call(it=items(capacity=bounds[1] - 1)) == BOUNDS and call(it=items(reserved=1)) == INVALID
    assert call(it=items(capacity=0), lo=3) == BOUNDS  # the items before the bounds
    assert call(lo=3) == INVALID and call(hi=1) == INVALID and call(lo=8, hi=6) == INVALID
    assert call(out=results(size=C.sizeof(QualityResult) - 8)) == INVALID
    assert call(lo=3, count=0) == INVALID and call(count=0) == 0  # the bound rules hold for an empty list too
    assert host(gpu.ctx, n, items(), SIZE, 1, None, 0, 0, 0, 1, res) == NULL_ and host(gpu.ctx, n, items(), SIZE, 1, limits, 0, 0, 0, 1, None) == NULL_
    torch.cuda.synchronize()
    assert all(int((r != 0x5A).sum()) == 0 for r in room), "a refused call wrote to an output buffer"
    assert all(r.errorFactor == 0x5A5A and r.bytes == 0x5A5A for r in res), "a refused call wrote to a result"
    assert call() == 0 and all(r.errorFactor % 2 == 0 and 2 <= r.errorFactor <= 1024 and r.bytes <= b for r, b in zip(res, bounds))
    gpu.check()


def test_host_form_capacity_rule(gpu, oracle):
    """a capacity below that result's bytes: all results are filled, no stream is written, OutOfBounds"""
    shapes = EDGES[:3]
    imgs = [np.ascontiguousarray(i) for i in _images(oracle, shapes)]
    limits = _limits(gpu, shapes)
    want, wres = gpu.encode_stream_quality_list(imgs, True, limits)
    outs = [np.full(s.size, 0x5A, dtype=np.uint8) for s in want]
    it = (StreamListItem * len(imgs))()
    for k, (i, o) in enumerate(zip(imgs, outs)):
        it[k] = StreamListItem(i.ctypes.data, o.ctypes.data, o.size - (1 if k == 1 else 0), i.shape[1], i.shape[0], 0, 0)
    res = (QualityResult * len(imgs))()
    for r in res:
        r.struct_size = C.sizeof(QualityResult)
    lim = (C.c_uint64 * len(imgs))(*limits)
    assert gpu.lib.limg_hip_encode_stream_quality_list(gpu.ctx, len(imgs), it, C.sizeof(StreamListItem), 1, lim, 0, 0, 0, 1, res) == 103
    assert [r.bytes for r in res] == [r.bytes for r in wres] and all(int((o != 0x5A).sum()) == 0 for o in outs)
    it[1].capacity = outs[1].size
    assert gpu.lib.limg_hip_encode_stream_quality_list(gpu.ctx, len(imgs), it, C.sizeof(StreamListItem), 1, lim, 0, 0, 0, 1, res) == 0
    assert all(np.array_equal(o, s) for o, s in zip(outs, want))


L.product_twins(globals())  # test_x_product: the same tests on the product library (tests/lib_axis.py)
