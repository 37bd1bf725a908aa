"""limg_hip_stream_sizes_list(_device): the sizes limg_hip_encode_stream would report for every image of a list of MIXED shapes at every entry of a list of error
factors, without encoding -- per chunk one k_fit_tpb_list grid, then one k_rate_probe_list launch and one step (its list form: sizes[image][factor]) per factor, one
download.  Every entry must equal the CPU oracle's size (tests/rate_search.py) and the length of limg_hip_encode_stream's stream; the lists are those of
tests/test_gpu_stream_budget_list.py that reach the probe's edges (`edges`), three channels (`rgb`) and the single call inside the same call (`ragged_inside`)."""
import ctypes as C

import numpy as np
import pytest

import lib_axis as L
from budget_list_cases import LISTS, image as _image
from lib_axis import lib, lib_product  # noqa: F401  (fixtures: "test" / "product")
from limg_amd import StreamListItem
from rate_search import oracle_size

pytestmark = pytest.mark.gpu

FACTORS = (0, 1, 2, 37, 101, 400, 1000)
NAMES = ("edges", "rgb", "ragged_inside")


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


@pytest.fixture(scope="module")
def lists(oracle):
    """(images, alpha, the oracle's sizes [image][factor]) of every list, computed once"""
    out = {}
    for name in NAMES:
        alpha, shapes, kw = LISTS[name]
        imgs = [_image(oracle, w, h, i) for i, (w, h) in enumerate(shapes)]
        out[name] = (imgs, alpha, np.array([[oracle_size(oracle, img, alpha, ef) for ef in FACTORS] for img in imgs], dtype=np.uint64))
    return out


def _to_device(imgs):
    import torch
    return [torch.from_numpy(i.view(np.int32)).cuda() for i in imgs]


@pytest.mark.parametrize("name", NAMES)
def test_sizes_against_the_oracle_and_the_encode(gpu, lists, name):
    """the host form and the device form (items with pStream = NULL and capacity = 0), 7 factors and 1"""
    imgs, alpha, want = lists[name]
    got = gpu.stream_sizes_list(imgs, alpha, FACTORS)
    print(name, got.tolist(), want.tolist())
    assert got.shape == want.shape and np.array_equal(got, want), name
    own = np.array([[gpu.encode_stream(img, alpha, error_factor=ef).size for ef in FACTORS] for img in imgs], dtype=np.uint64)
    assert np.array_equal(got, own), name
    dimgs = _to_device(imgs)
    assert np.array_equal(gpu.stream_sizes_list_device(dimgs, alpha, FACTORS), want), (name, "device")
    assert np.array_equal(gpu.stream_sizes_list(imgs, alpha, FACTORS[3:4]), want[:, 3:4]), (name, "one factor")
    assert np.array_equal(gpu.stream_sizes_list_device(dimgs, alpha, FACTORS[5:6]), want[:, 5:6]), (name, "one factor, device")
    gpu.check()


def test_chunks(gpu, lists):
    """test hook batch_chunk = 3: edges as 3 + 3 + 1, the last through the single call"""
    if not L.has_hooks(gpu):
        return
    imgs, alpha, want = lists["edges"]
    gpu.set_options(test_batch_chunk=3)
    try:
        for rep in range(2):
            assert np.array_equal(gpu.stream_sizes_list(imgs, alpha, FACTORS), want), rep
    finally:
        gpu.set_options()


def test_single_calls_and_empty_lists(gpu, lists):
    imgs, alpha, want = lists["edges"]
    for i in (0, 4):
        assert gpu.stream_sizes(imgs[i], alpha, FACTORS) == want[i].tolist()
    assert np.array_equal(gpu.stream_sizes_list(imgs[:1], alpha, FACTORS), want[:1])
    assert gpu.stream_sizes_list([], alpha, FACTORS).shape == (0, len(FACTORS)) and gpu.stream_sizes_list(imgs, alpha, []).shape == (len(imgs), 0)


def test_errors(gpu):
    """the refusals, in the contract's order, before anything touches the device: pBytes keeps its pattern; pStream and capacity are not looked at"""
    import torch
    shapes = ((64, 16), (8, 8), (264, 24))
    n, m = len(shapes), 2
    imgs = [torch.zeros((h, w), dtype=torch.int32, device="cuda") for w, h in shapes]
    dev, host = gpu.lib.limg_hip_stream_sizes_list_device, gpu.lib.limg_hip_stream_sizes_list
    NULL_, INVALID = 102, 101  # limg_hip_error_ArgumentNull, _InvalidParameter
    SIZE = C.sizeof(StreamListItem)
    efs = (C.c_uint32 * m)(100, 7)
    sizes = (C.c_size_t * (n * m))(*([0x5A5A] * (n * m)))

    def items(**change):
        it = (StreamListItem * n)()
        for k in range(n):
            it[k] = StreamListItem(imgs[k].data_ptr(), None, 0, shapes[k][0], shapes[k][1], 0, 0)
        for name, v in change.items():
            setattr(it[1], name, v)
        return it

    def call(ctx=gpu.ctx, count=n, it=None, size=SIZE, pe=efs, factors=m, pb=sizes):
        return dev(ctx, count, items() if it is None else it, size, 1, pe, factors, pb, 0, 1, None)

    assert call(ctx=None) == NULL_ and call(pe=None) == NULL_ and call(pb=None) == NULL_ and dev(gpu.ctx, n, None, SIZE, 1, efs, m, sizes, 0, 1, None) == NULL_
    assert call(count=0, pb=None) == NULL_ and call(factors=0, pe=None) == NULL_
    assert call(size=SIZE - 1) == INVALID and call(size=0, it=items(pIn=None)) == INVALID
    assert call(it=items(pIn=None)) == NULL_ and call(it=items(sizeX=0)) == INVALID and call(it=items(sizeY=0)) == INVALID
    assert call(it=items(sizeX=0xFFFFFFF8, sizeY=0xFFFFFFF8)) == INVALID and call(it=items(reserved=1)) == INVALID
    assert call(it=items(pIn=None, reserved=1)) == NULL_ and call(it=items(reserved=1), factors=0) == INVALID
    assert host(None, n, items(), SIZE, 1, efs, m, sizes, 0, 1) == NULL_ and host(gpu.ctx, n, items(), SIZE, 1, efs, m, None, 0, 1) == NULL_
    assert host(gpu.ctx, n, items(reserved=3), SIZE, 1, efs, m, sizes, 0, 1) == INVALID
    # an empty list, or an empty list of factors: success with nothing done
    assert call(count=0) == 0 and call(factors=0) == 0 and host(gpu.ctx, 0, items(), SIZE, 1, efs, m, sizes, 0, 1) == 0
    assert list(sizes) == [0x5A5A] * (n * m), "a refused call wrote to pBytes"
    # the same arguments are accepted; an odd pStream and a capacity are ignored
    assert call(it=items(pStream=12345, capacity=3, errorFactor=77)) == 0
    flat = [[gpu.encode_stream(np.zeros((h, w), dtype=np.uint32), True, error_factor=ef).size for ef in efs] for w, h in shapes]
    assert list(sizes) == [v for row in flat for v in row]
    gpu.check()


def test_context_memory(lib, lists):
    """the probe's share of a mixed-list encode (tables, records, invN, look-back words), a state and a counter per image, 8 x factors per image + 4 x factors of
    list; a second call grows nothing"""
    imgs, alpha, want = lists["edges"]
    dimgs = _to_device(imgs)
    n, m = len(imgs), len(FACTORS)
    up = lambda v, a: (v + a - 1) // a * a  # noqa: E731
    blocks = sum((i.shape[0] // 8) * (i.shape[1] // 8) for i in imgs)
    strips = sum((i.shape[0] // 8) * ((i.shape[1] // 8 + 31) // 32) for i in imgs)
    tables = 0
    for entry in (160, 64, 96, 32, 32, 4, 4):  # view, ListImage, ImageIO, RatedImage, StreamImage, two prefix words
        tables = up(tables + n * entry, 16)
    stated = tables + blocks * (64 + 16) + 32 + 8 * strips + (72 + 8) * n + 8 * m * n + 4 * m
    g = L.open_context(lib)
    try:
        base = g.device_bytes()
        assert np.array_equal(g.stream_sizes_list_device(dimgs, alpha, FACTORS), want)
        held = g.device_bytes()
        assert held - base == stated, (held, base, stated)
        g.stream_sizes_list_device(dimgs, alpha, FACTORS[:3])
        assert g.device_bytes() == held
        g.check()
    finally:
        g.close()


L.product_twins(globals())  # test_x_product: the same tests on the product library (tests/lib_axis.py)
