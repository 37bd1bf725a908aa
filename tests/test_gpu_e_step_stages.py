"""The E step's stages (fit_search_strip's callees in limg_hip_kernels.hip / limg_hip_float_pixel.h), the chain partition helpers (chain_of_row / chain_head_row) and
the shared factor-plane copy (copy_factor_planes), on the smallest shapes at which each can go wrong.  Every plane and the compact outputs bit-identical to the oracle
for the 16 EXACT instances of the E step: {3, 4 channels} x {fused, force_split} x {k_fit_tpb, legacy_float_stage} x {default, accurate search}, on both libraries.
(The FAST float instances have no bit-exact oracle: tests/test_gpu_fast_float.py checks all of them.)

  264 x 16          two strips per block row, the second with one block: `bx >= blocksX` in the record load, the block queue and the factor copy; two block rows, so a
                    look-back looks back
  272 x 16          width a multiple of 16: the 16-byte form of the factor-plane copy with a partial second strip (split path)
  264 x 48, pool 2  two chains of three block rows: the chain head in the publish, the look-back and k_strip_scan
  61 x 27, 3 x 1    partial blocks both ways; 3 x 1 is a block of fewer than 4 pixels (chain_head_row in the float stage's gather rule).  Ragged images always run
                    the lane == pixel float stage, so these run once per (channels, path, search)
  260 x 8, + 4 B    every device pointer 4 bytes past a 16-byte boundary: the dword form of the pixel staging, the bytewise form of the factor-plane copy
  264 x 16 compact  records + shift words + the three factor planes only"""
import numpy as np
import pytest

import lib_axis as L
from oracle.bind import PLANES, REC_DTYPE

pytestmark = pytest.mark.gpu

WHOLE = (("264x16", 264, 16, 0), ("272x16", 272, 16, 0), ("264x48 pool 2", 264, 48, 2), ("260x8", 260, 8, 0))
RAGGED = (("61x27", 61, 27), ("3x1", 3, 1))


def _ctx(lib):
    g = L.open_context(lib)
    yield g
    g.check()
    g.close()


@pytest.fixture(scope="module")
def gpu():
    yield from _ctx("test")


@pytest.fixture(scope="module")
def gpu_product():
    yield from _ctx("product")


@pytest.fixture(scope="module")
def wanted(oracle):
    """{(name, alpha, fast): (image, the oracle's planes and extras)}, computed once for every instance and both libraries"""
    big = oracle.photo_noise(272, 48, 23)
    out = {}
    for alpha in (True, False):
        for fast in (True, False):
            for name, w, h, pool in WHOLE:
                img = np.ascontiguousarray(big[:h, :w])
                out[name, alpha, fast] = (img, oracle.encode3d(img, alpha, extras=(name == "264x16"), error_factor=100, fast=fast, pool_threads=pool))
            for name, w, h in RAGGED:
                img = np.ascontiguousarray(big[:h, :w])
                out[name, alpha, fast] = (img, oracle.encode3d(img, alpha, error_factor=100, fast=fast))
    return out


def _host(planes):
    import torch
    return {k: v.cpu().numpy().view(np.uint32 if v.dtype == torch.int32 else np.uint8) for k, v in planes.items()}


def _assert_planes(got, want, ctx, names=PLANES):
    bad = [(k, int((got[k] != want[k]).sum())) for k in names if not np.array_equal(got[k], want[k])]
    assert not bad, (ctx, bad)


def _offset_tensor(h, w, dtype, skip):
    """an (h, w) device tensor whose first element lies `skip` elements into a fresh (16-byte aligned) allocation"""
    import torch
    return torch.zeros(w * h + 32, dtype=dtype, device="cuda")[skip:skip + w * h].view(h, w)


@pytest.mark.parametrize("search", ["default", "accurate"])
@pytest.mark.parametrize("stage", ["tpb", "legacy"])
@pytest.mark.parametrize("path", ["fused", "split"])
@pytest.mark.parametrize("channels", [4, 3])
def test_e_step_instance_is_bit_identical_to_the_oracle(gpu, wanted, channels, path, stage, search):
    import torch
    import limg_amd
    alpha, fast = channels == 4, search == "default"
    gpu.set_options(force_split=(path == "split"), legacy_float_stage=(stage == "legacy"))
    ctx = (channels, path, stage, search)
    for name, w, h, pool in WHOLE:
        img, want = wanted[name, alpha, fast]
        skip = 1 if name == "260x8" else 0  # 4 bytes: one pixel / plane dword, four factor bytes
        d_img = _offset_tensor(h, w, torch.int32, skip)
        d_img.copy_(torch.from_numpy(img.view(np.int32)))
        planes = {k: _offset_tensor(h, w, torch.uint8 if k in limg_amd.P8 else torch.int32, 4 * skip if k in limg_amd.P8 else skip) for k in PLANES}
        assert all(t.data_ptr() % 16 == 4 * skip for t in list(planes.values()) + [d_img])
        gpu.encode3d_device(d_img, alpha, planes, error_factor=100, pool_threads=pool, fast=fast)
        torch.cuda.synchronize()
        _assert_planes(_host(planes), want, ctx + (name,))
    if stage == "tpb":  # (ragged images never take the records of k_fit_tpb: one run per (channels, path, search))
        for name, w, h in RAGGED:
            img, want = wanted[name, alpha, fast]
            _assert_planes(gpu.encode3d(img, alpha, error_factor=100, fast=fast), want, ctx + (name,))
    # compact mode: the three factor planes, records and shift words
    img, want = wanted["264x16", alpha, fast]
    w, h, bx, by = 264, 16, 33, 2
    fac = {k: torch.zeros((h, w), dtype=torch.uint8, device="cuda") for k in limg_amd.P8}
    rec = torch.zeros((by * bx, 16), dtype=torch.int32, device="cuda")
    sh = torch.zeros(by * bx, dtype=torch.int32, device="cuda")
    gpu.encode3d_device(torch.from_numpy(img.view(np.int32)).cuda(), alpha, fac, error_factor=100, fast=fast, records=rec, shifts=sh)
    torch.cuda.synchronize()
    _assert_planes(_host(fac), want, ctx + ("compact",), limg_amd.P8)
    grec = rec.cpu().numpy().view(REC_DTYPE).reshape(by, bx)
    for f in REC_DTYPE.names:
        assert np.array_equal(grec[f], want["records"][f]), ctx + ("compact records", f)
    gsh = sh.cpu().numpy().astype(np.uint32).reshape(by, bx)
    for i in range(3):
        assert np.array_equal((gsh >> (8 * i)) & 0xFF, want["shifts"][:, :, i]), ctx + ("compact shift", i)


L.product_twins(globals())
