"""The persistent encode kernel's per-strip bookkeeping on the GPU: what a work strip knows of itself (its image, block row, park slot, the strips of the launch, its
place in the dither chain) is fetched or worked out again where a stage uses it, not carried across the search.  None of it may change a result bit, so every case
is all 11 planes against the CPU oracle, in 4 and 3 channels at errorFactor 100:
 * widths 8, 248, 256, 264 and 520 -- one block; a strip one block short; exactly one strip; one block into a second strip; three strips with a short last one --
   at heights 8 and 24 (one block row, three);
 * 264x24 with pool_threads=2: two dither chains, the second restarted at block row 1;
 * three 264x16 images in one batched call: the strips' image comes from the launch's image table;
 * 520x24 through the split path (`force_split`), which shares the E and F steps' code.
All sizes are whole blocks (images with partial blocks do not run the persistent kernel).  On the test build and on the product library."""
import numpy as np
import pytest

import lib_axis as L
from lib_axis import lib, lib_product  # noqa: F401  (fixtures: "test" / "product")
from oracle.bind import PLANES

pytestmark = pytest.mark.gpu

WIDTHS = (8, 248, 256, 264, 520)
HEIGHTS = (8, 24)
ERROR_FACTOR = 100


@pytest.fixture(scope="module")
def wanted(oracle):
    """the inputs and the oracle's planes, computed once for every test and both libraries"""
    big = oracle.photo_noise(520, 24, 23)
    out = {"shapes": [], "chains": [], "batch": [], "split": []}
    for alpha in (True, False):
        for w in WIDTHS:
            for h in HEIGHTS:
                img = np.ascontiguousarray(big[:h, :w])
                out["shapes"].append(("%dx%d alpha=%s" % (w, h, alpha), img, alpha, oracle.encode3d(img, alpha, error_factor=ERROR_FACTOR)))
        img = np.ascontiguousarray(big[:24, :264])
        out["chains"].append(("264x24 pool_threads=2 alpha=%s" % alpha, img, alpha, oracle.encode3d(img, alpha, error_factor=ERROR_FACTOR, pool_threads=2)))
        imgs = [np.ascontiguousarray(oracle.photo_noise(264, 16, 31 + i)) for i in range(3)]
        out["batch"].append(("3 x 264x16 alpha=%s" % alpha, imgs, alpha, [oracle.encode3d(i, alpha, error_factor=ERROR_FACTOR) for i in imgs]))
        img = np.ascontiguousarray(big[:24, :520])
        out["split"].append(("520x24 split alpha=%s" % alpha, img, alpha, oracle.encode3d(img, alpha, error_factor=ERROR_FACTOR)))
    return out


def to_host(planes):
    import torch
    return {k: v.cpu().numpy().view(np.uint32 if v.dtype == torch.int32 else np.uint8) for k, v in planes.items()}


def upload(img):
    import torch
    return torch.from_numpy(img.view(np.int32)).cuda()


def encode(g, img, alpha, **kw):
    import torch
    h, w = img.shape
    planes = g.alloc_planes_device(w, h)
    g.encode3d_device(upload(img), alpha, planes, error_factor=ERROR_FACTOR, **kw)
    torch.cuda.synchronize()
    return to_host(planes)


def differing(got, want):
    assert len(PLANES) == 11
    return [(k, int((got[k] != want[k]).sum())) for k in PLANES if not np.array_equal(got[k], want[k])]


def test_strip_shapes_are_bit_identical_to_the_oracle(lib, wanted):
    g = L.open_context(lib)
    try:
        assert len(wanted["shapes"]) == 2 * len(WIDTHS) * len(HEIGHTS)
        for name, img, alpha, want in wanted["shapes"]:
            bad = differing(encode(g, img, alpha), want)
            assert not bad, (name, bad)
        g.check()
    finally:
        g.close()


def test_restarted_chains_are_bit_identical_to_the_oracle(lib, wanted):
    g = L.open_context(lib)
    try:
        for name, img, alpha, want in wanted["chains"]:
            bad = differing(encode(g, img, alpha, pool_threads=2), want)
            assert not bad, (name, bad)
        g.check()
    finally:
        g.close()


def test_batched_call_is_bit_identical_to_the_oracle(lib, wanted):
    import torch
    g = L.open_context(lib)
    try:
        for name, imgs, alpha, wants in wanted["batch"]:
            outs = [g.alloc_planes_device(264, 16) for _ in imgs]
            g.encode3d_batch_device([upload(i) for i in imgs], alpha, outs, error_factor=ERROR_FACTOR)
            torch.cuda.synchronize()
            for i, (out, want) in enumerate(zip(outs, wants)):
                bad = differing(to_host(out), want)
                assert not bad, (name, i, bad)
        g.check()
    finally:
        g.close()


def test_split_path_is_bit_identical_to_the_oracle(lib, wanted):
    g = L.open_context(lib)
    try:
        g.set_options(force_split=True)
        for name, img, alpha, want in wanted["split"]:
            bad = differing(encode(g, img, alpha), want)
            assert not bad, (name, bad)
        g.check()
    finally:
        g.close()


L.product_twins(globals())
