"""k_compare (limg_hip_compare / limg_hip_compare_device == the reference's limg_compare) against the oracle on pairs that are NOT an image and its own decode:
those practically never have a red difference of 128 or more, so the branch that swaps the red and blue weights never ran.  The error sum is compared exactly
(as mse x pixel count: an integer well below 2^53), the PSNR to the suite's 1e-9; for zero error whatever the oracle returns is the expectation."""
import math

import numpy as np
import pytest

import lib_axis as L

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1), (3, 1), (61, 27), (264, 16)]  # w x h


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


def _pairs(w, h):
    rng = np.random.default_rng(w * 1000 + h)
    a, b = (rng.integers(0, 2 ** 32, (h, w), dtype=np.uint32) for _ in range(2))
    alpha_only = a ^ (rng.integers(1, 256, (h, w), dtype=np.uint32) << 24)
    red_edge = a & 0xFFFFFF00
    red_edge_b = red_edge | rng.choice(np.array([126, 127, 128, 129, 255], dtype=np.uint32), (h, w))  # a red difference on both sides of 128 (its square: 0x4000)
    return {"random": (a, b), "itself": (a, a), "extremes": (np.zeros((h, w), np.uint32), np.full((h, w), 0xFFFFFFFF, np.uint32)), "alpha_only": (a, alpha_only),
            "red_edge": (red_edge, red_edge_b)}


def _same(got, want, n, ctx):
    (gp, gm), (wp, wm) = got, want
    assert round(gm * n) == round(wm * n) and gm == wm, (ctx, gm * n, wm * n)
    if math.isinf(wp) or math.isnan(wp):
        assert gp == wp or (math.isnan(gp) and math.isnan(wp)), (ctx, gp, wp)
    else:
        assert gp == pytest.approx(wp, abs=1e-9), (ctx, gp, wp)


@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("alpha", [True, False], ids=["ch4", "ch3"])
def test_compare_pairs(gpu, oracle, w, h, alpha):
    import torch
    for name, (a, b) in _pairs(w, h).items():
        want = oracle.compare(a, b, alpha)
        if name == "itself":
            assert want[1] == 0.0
        if name == "alpha_only":
            assert (want[1] == 0.0) == (not alpha)  # 3 channels: alpha does not count
        _same(gpu.compare(a, b, alpha), want, w * h, (name, "host"))
        da, db = (torch.from_numpy(x.view(np.int32)).cuda() for x in (a, b))
        _same(gpu.compare_device(da, db, alpha), want, w * h, (name, "device"))
        # device pointers offset by 4 bytes
        bufs = [torch.zeros(w * h + 8, dtype=torch.int32, device="cuda") for _ in range(2)]
        off = [buf[1:1 + w * h].view(h, w) for buf in bufs]
        off[0].copy_(da)
        off[1].copy_(db)
        assert all(t.data_ptr() % 8 == 4 for t in off)
        _same(gpu.compare_device(off[0], off[1], alpha), want, w * h, (name, "device + 4 bytes"))


L.product_twins(globals())
