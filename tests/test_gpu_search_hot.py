"""The generated straight-line hot subtree of the default shift search (limg_search_hot.h) on the GPU: the inputs that reach every hot state and both of its edges
(tests/search_hot_inputs.py; tests/test_search_hot.py holds that condition on the CPU) through the persistent kernel and through the split path (`force_split`), on
the test build and on the product library, all 11 planes bit-identical to the oracle.  One 508x64 image adds partial blocks, which take the untouched table loop, next
to whole blocks."""
import numpy as np
import pytest

import lib_axis as L
from lib_axis import lib, lib_product  # noqa: F401  (fixtures: "test" / "product")
import search_hot_inputs as inputs
from oracle.bind import PLANES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def wanted(oracle):
    """[(name, image, has_alpha, errorFactor, the oracle's planes)], computed once for both paths and both libraries"""
    out = []
    for i, (img, alpha, ef) in enumerate(inputs.coverage_inputs(oracle)):
        out.append(("input %d (%dx%d, alpha=%s, errorFactor %d)" % (i, img.shape[1], img.shape[0], alpha, ef), img, alpha, ef, oracle.encode3d(img, alpha, error_factor=ef)))
    img = inputs.image(oracle, "photo_noise", 508, 64)
    for alpha in (True, False):
        out.append(("508x64 alpha=%s" % alpha, img, alpha, 100, oracle.encode3d(img, alpha, error_factor=100)))
    return out


@pytest.mark.parametrize("mode", ["persistent", "split"])
def test_hot_search_inputs_are_bit_identical_to_the_oracle(lib, wanted, mode):
    import torch
    g = L.open_context(lib)
    try:
        g.set_options(force_split=(mode == "split"))
        for name, img, alpha, ef, want in wanted:
            h, w = img.shape
            if w % 8 == 0:
                planes = g.alloc_planes_device(w, h)
                g.encode3d_device(torch.from_numpy(img.view(np.int32)).cuda(), alpha, planes, error_factor=ef)
                torch.cuda.synchronize()
                got = {k: v.cpu().numpy().view(np.uint32 if v.dtype == torch.int32 else np.uint8) for k, v in planes.items()}
            else:
                got = g.encode3d(img, alpha, error_factor=ef)
            bad = [(k, int((got[k] != want[k]).sum())) for k in PLANES if not np.array_equal(got[k], want[k])]
            assert len(PLANES) == 11 and not bad, (name, mode, bad)
        g.check()
    finally:
        g.close()


L.product_twins(globals())
