"""EXACT float stage, bit for bit against the oracle, on inputs PROVEN to reach its edges (tests/float_edge_inputs.py, tests/test_float_edges.py): skipped pixels,
signs decided by the preference bias, exact ties of every lane pair, zero and NaN directions, record fields from NaN and from k + 0.5, factors beyond the clamp,
all 2 048 RSQRTPS table indices and arguments down to 2^-106.  The EXACT contract has no exception for degenerate blocks.

What runs what (fixture modes as in tests/test_gpu_fast_float.py):
  test_whole_blocks            k_fit_tpb (fused, split) / the E step's lane == pixel stage (legacy, split_legacy), 3 and 4 channels, default and accurate search
  test_whole_blocks_unaligned  the same from a 4-byte-aligned input: k_fit_tpb<DIRECT = false> / the E step's dword staging
  test_partial_blocks          lane == pixel on partial edge blocks: the cropped image (last column 5 wide, last row 3 high), a height-only crop (fused: both stages
                               in one image; with the whole-image ragged hook: every block lane == pixel) and the 1x1, 3x1, 2x65 shapes (blocks of fewer than 4 pixels)
  test_merged_blocks           the merged-block encoder's per-block and region fits: rectangles, then every written plane
  test_stream_sizes            k_rate_probe's own factor computation: sizes at errorFactor 0 / 2 / 100 / 400 against the CPU restatement of the container
  test_batch_list              the float-stage grid over a list: the image and the image rolled by one block row
Records and shift words are compared first, field by field, so a failure names the block and the field; then all 11 planes."""
import numpy as np
import pytest

import float_edge_inputs as F
import lib_axis as L
import rate_search as R
from lib_axis import lib, lib_product  # noqa: F401  (fixtures: "test" / "product")
from oracle.bind import BLOCKED_WRITTEN, PLANES, REC_DTYPE

pytestmark = pytest.mark.gpu
MODES = ["fused", "split", "legacy", "split_legacy"]


def _gpu(mode, lib):
    g = L.open_context(lib)
    g.mode = mode
    plain = g.set_options

    def set_options(**kw):  # every options change inside a test keeps the fixture's mode
        kw.setdefault("force_split", mode in ("split", "split_legacy"))
        kw.setdefault("legacy_float_stage", mode in ("legacy", "split_legacy"))
        plain(**kw)
    g.set_options = set_options
    g.set_options()
    yield g
    g.set_options()
    g.check()
    g.close()


@pytest.fixture(scope="module", params=MODES)
def gpu(request):
    yield from _gpu(request.param, "test")


@pytest.fixture(scope="module", params=MODES)
def gpu_product(request):
    yield from _gpu(request.param, "product")


_IMAGES, _WANT = {}, {}


def _image(name):
    if not _IMAGES:
        tiny = F.tiny_images()
        whole = F.whole_image()
        _IMAGES.update(whole=whole, cropped=F.cropped_image(), cropped_h=np.ascontiguousarray(whole[:-5]), tiny1x1=tiny[0], tiny3x1=tiny[1], tiny2x65=tiny[2],
                       rolled=np.ascontiguousarray(np.roll(whole, 8, axis=0)), merged=F.merged_image())
    return _IMAGES[name]


def _want(oracle, name, alpha, fast=True, ef=100):
    """the oracle's encode, computed once per case and shared (never modified)"""
    key = (name, alpha, fast, ef)
    if key not in _WANT:
        _WANT[key] = oracle.encode3d(_image(name), alpha, extras=True, fast=fast, error_factor=ef)
    return _WANT[key]


def _encode(gpu, d_img, alpha, fast=True, **opts):
    import torch
    h, w = d_img.shape
    gpu.set_options(**opts)
    planes = gpu.alloc_planes_device(w, h)
    by, bx = (h + 7) // 8, (w + 7) // 8
    rec = torch.zeros((by * bx, 16), dtype=torch.int32, device="cuda")
    sh = torch.zeros(by * bx, dtype=torch.int32, device="cuda")
    try:
        gpu.encode3d_device(d_img, alpha, planes, records=rec, shifts=sh, fast=fast)
        torch.cuda.synchronize()
    finally:
        gpu.set_options()
    out = {k: v.cpu().numpy().view(np.uint32 if v.dtype == torch.int32 else np.uint8) for k, v in planes.items()}
    out["records"] = rec.cpu().numpy().view(REC_DTYPE).reshape(by, bx)
    out["shifts"] = sh.cpu().numpy().astype(np.uint32).reshape(by, bx)
    return out


def _dev(img):
    import torch
    return torch.from_numpy(np.ascontiguousarray(img).view(np.int32)).cuda()


def _check(got, want, ctx):
    """records (bit patterns: avg as its 32 bits), shift words, then the planes; the first differing blocks are named as (block row, block column, lane)"""
    for f in REC_DTYPE.names:
        g, w = got["records"][f], want["records"][f]
        if f == "avg":
            g, w = g.view(np.uint32), w.view(np.uint32)
        assert np.array_equal(g, w), (ctx, "record", f, "blocks", np.argwhere(g != w)[:6].tolist(), g[g != w][:6].tolist(), w[g != w][:6].tolist())
    for i in range(3):
        g, w = (got["shifts"] >> (8 * i)) & 0xFF, want["shifts"][:, :, i]
        assert np.array_equal(g, w), (ctx, "shift", i, "blocks", np.argwhere(g != w)[:6].tolist())
    bad = [(k, int((got[k] != want[k]).sum()), np.argwhere(got[k] != want[k])[:3].tolist()) for k in PLANES if not np.array_equal(got[k], want[k])]
    assert not bad, (ctx, bad)


@pytest.mark.parametrize("fast", [True, False], ids=["default", "accurate"])
@pytest.mark.parametrize("alpha", [True, False], ids=["ch4", "ch3"])
def test_whole_blocks(gpu, oracle, alpha, fast):
    _check(_encode(gpu, _dev(_image("whole")), alpha, fast), _want(oracle, "whole", alpha, fast), (gpu.mode, alpha, fast))


@pytest.mark.parametrize("alpha", [True, False], ids=["ch4", "ch3"])
def test_whole_blocks_unaligned(gpu, oracle, alpha):
    import torch
    img = _image("whole")
    h, w = img.shape
    buf = torch.zeros(w * h + 8, dtype=torch.int32, device="cuda")
    d_img = buf[1:1 + w * h].view(h, w)
    d_img.copy_(torch.from_numpy(img.view(np.int32)))
    assert d_img.data_ptr() % 16 == 4
    _check(_encode(gpu, d_img, alpha), _want(oracle, "whole", alpha), (gpu.mode, alpha, "unaligned"))


@pytest.mark.parametrize("name", ["cropped", "cropped_h", "tiny1x1", "tiny3x1", "tiny2x65"])
@pytest.mark.parametrize("alpha", [True, False], ids=["ch4", "ch3"])
def test_partial_blocks(gpu, oracle, alpha, name):
    d_img = _dev(_image(name))
    want = _want(oracle, name, alpha)
    _check(_encode(gpu, d_img, alpha), want, (gpu.mode, alpha, name))
    if L.has_hooks(gpu):
        _check(_encode(gpu, d_img, alpha, test_whole_image_ragged=True), want, (gpu.mode, alpha, name, "whole-image ragged"))


@pytest.mark.parametrize("alpha", [True, False], ids=["ch4", "ch3"])
def test_merged_blocks(lib, oracle, alpha):
    g = L.open_context(lib)
    try:
        img = _image("merged")
        want = oracle.blocked_encode3d(img, alpha)
        assert int((want["regions"]["rx"] * want["regions"]["ry"]).max()) > 1  # the rectangles made to merge did merge
        got = g.blocked_encode3d(img, alpha)
        wr, gr = want["regions"], got["regions"]
        assert len(wr) == len(gr), (alpha, len(wr), len(gr))
        for f in ("ox", "oy", "rx", "ry"):
            assert np.array_equal(wr[f], gr[f]), (alpha, f, np.argwhere(wr[f] != gr[f])[:4].ravel())
        bad = [(k, int((got[k] != want[k]).sum()), np.argwhere(got[k] != want[k])[:3].tolist()) for k in BLOCKED_WRITTEN if not np.array_equal(got[k], want[k])]
        assert not bad, (alpha, bad)
        g.check()
    finally:
        g.close()


@pytest.mark.parametrize("alpha", [True, False], ids=["ch4", "ch3"])
def test_stream_sizes(lib, oracle, alpha):
    g = L.open_context(lib)
    try:
        img = _image("whole")
        efs = [0, 2, 100, 400]
        want = [R.oracle_size(oracle, img, alpha, ef) for ef in efs]
        assert g.stream_sizes(img, alpha, efs) == want
        assert g.stream_sizes_device(_dev(img), alpha, efs) == want
        g.check()
    finally:
        g.close()


@pytest.mark.parametrize("alpha", [True, False], ids=["ch4", "ch3"])
def test_batch_list(gpu, oracle, alpha):
    import torch
    names = ("whole", "rolled")
    imgs = [_dev(_image(n)) for n in names]
    h, w = imgs[0].shape
    planes = [gpu.alloc_planes_device(w, h) for _ in names]
    gpu.encode3d_batch_device(imgs, alpha, planes)
    torch.cuda.synchronize()
    for n, pl in zip(names, planes):
        want = _want(oracle, n, alpha)
        got = {k: v.cpu().numpy().view(np.uint32 if v.dtype == torch.int32 else np.uint8) for k, v in pl.items()}
        bad = [(k, int((got[k] != want[k]).sum()), np.argwhere(got[k] != want[k])[:3].tolist()) for k in PLANES if not np.array_equal(got[k], want[k])]
        assert not bad, (gpu.mode, alpha, n, bad)


L.product_twins(globals())
