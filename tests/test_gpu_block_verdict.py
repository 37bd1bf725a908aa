"""The block-sum verdict of the default shift search on the GPU (wave_sum_below: one lane's compare instead of the sum's value) and the trial tails around it:
 * whole blocks with a trial whose block sum is exactly blockLimit - 1 (passes) or exactly blockLimit (fails) -- tests/block_verdict_inputs.py; tests/test_block_verdict.py
   holds that condition on the CPU;
 * small shapes: one block, exactly one work strip, a second strip of one block over three block rows, 512x64, and partial blocks (the masked copy of the table loop),
   each in 3 and 4 channels at errorFactor 0, 25, 100 and 400;
 * the accurate search, which keeps the sum's value, on 512x64 and 13x11.
Through the persistent kernel and through the split path (`force_split`), on the test build and on the product library, all 11 planes bit-identical to the oracle."""
import numpy as np
import pytest

import lib_axis as L
from lib_axis import lib, lib_product  # noqa: F401  (fixtures: "test" / "product")
import block_verdict_inputs as inputs
from oracle.bind import PLANES

pytestmark = pytest.mark.gpu

SHAPES = ((8, 8), (256, 8), (264, 24), (512, 64), (13, 11), (508, 64))  # (w, h)
ERROR_FACTORS = (0, 25, 100, 400)
ACCURATE_SHAPES = ((512, 64), (13, 11))


@pytest.fixture(scope="module")
def wanted(oracle):
    """{group: [(name, image, has_alpha, errorFactor, fast, the oracle's planes)]}, computed once for both paths and both libraries"""
    out = {"edge": [], "shapes": [], "accurate": []}
    for img, ef, kinds in inputs.edge_images():
        for alpha in (True, False):  # (the blocks have their edge trials in 4 channels; 3 channels is one more input)
            out["edge"].append(("edge blocks, errorFactor %d, alpha=%s" % (ef, alpha), img, alpha, ef, True, oracle.encode3d(img, alpha, error_factor=ef)))
    big = oracle.photo_noise(512, 64, 11)
    for w, h in SHAPES:
        img = np.ascontiguousarray(big[:h, :w])
        for alpha in (True, False):
            for ef in ERROR_FACTORS:
                out["shapes"].append(("%dx%d alpha=%s errorFactor %d" % (w, h, alpha, ef), img, alpha, ef, True, oracle.encode3d(img, alpha, error_factor=ef)))
    for w, h in ACCURATE_SHAPES:
        img = np.ascontiguousarray(big[:h, :w])
        for alpha in (True, False):
            out["accurate"].append(("accurate %dx%d alpha=%s" % (w, h, alpha), img, alpha, 100, False, oracle.encode3d(img, alpha, error_factor=100, fast=False)))
    return out


def encode(g, img, alpha, ef, fast):
    import torch
    h, w = img.shape
    if w % 8 or h % 8:
        return g.encode3d(img, alpha, error_factor=ef, fast=fast)
    planes = g.alloc_planes_device(w, h)
    g.encode3d_device(torch.from_numpy(img.view(np.int32)).cuda(), alpha, planes, error_factor=ef, fast=fast)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().view(np.uint32 if v.dtype == torch.int32 else np.uint8) for k, v in planes.items()}


@pytest.mark.parametrize("mode", ["persistent", "split"])
@pytest.mark.parametrize("group", ["edge", "shapes", "accurate"])
def test_block_verdict_inputs_are_bit_identical_to_the_oracle(lib, wanted, group, mode):
    g = L.open_context(lib)
    try:
        g.set_options(force_split=(mode == "split"))
        assert wanted[group]
        for name, img, alpha, ef, fast, want in wanted[group]:
            got = encode(g, img, alpha, ef, fast)
            bad = [(k, int((got[k] != want[k]).sum())) for k in PLANES if not np.array_equal(got[k], want[k])]
            assert len(PLANES) == 11 and not bad, (name, mode, bad)
        g.check()
    finally:
        g.close()


L.product_twins(globals())
